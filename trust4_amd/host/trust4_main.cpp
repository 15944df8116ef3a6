// trust4_amd/host/trust4_main.cpp -- `trust4-hip`: stage-1 driver with the command line and the on-disk
// inputs/outputs of the reference's `trust4` (main.cpp), running the hot path on the MI355X through the C ABI
// of include/trust4_hip.h:
//   * rough annotation of every distinct read            -> t4_annotate_rough        (main.cpp:1084-1120)
//   * greedy assembly (AddRead / RepeatAddRead / ...)    -> t4_assembler_*           (main.cpp:1583-1940)
// Everything else here is the reference's host-side read handling restated: FASTA/FASTQ input, mate
// read-through / merge (ProcessRead, main.cpp:224-449, AlignAlgo::IsMateOverlap), canonical 21-mer counting and
// quality trimming (KmerCount.hpp:64-97, 177-288), the read order (main.cpp:103-125), V/C trimming
// (main.cpp:1262-1464), the per-read AddRead parameters and good-candidate propagation (main.cpp:1583-1880),
// the rescue pass and the three output files. Written from the behaviour of those functions, not copied.
//
// Barcode mode (--barcode [--UMI]; main.cpp:797-842, 1123-1193, 1549-1559, 1846-1859): every cell is an independent
// contig set (t4_cellset), so the Add queries of many cells run in one launch ("lanes") while each cell's reads are
// committed in the reference's order; outputs are those of the reference's cell-after-cell pass.
// --keepNoBarcode (main.cpp:1556-1559): the index is not keyed by barcode then, so the reads go through ONE contig set
// with the barcode filter; --contigMinCov (main.cpp:822-828, 951-977, 1855, 1952-1955).
// Limits of this round: no -c/--debug-ns; without barcodes `_final.out` is written as a
// copy of `_raw.out` (the reference does the same under --skipMateExtension and always with barcodes; its mate-graph
// extension tail is out of scope).
#include <fcntl.h>
#include <sys/wait.h>
#include <spawn.h>
#include <functional>
#include <sys/stat.h>
#include <getopt.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/trust4_hip.h"
#include "process_read.h"
#include "seq_reader.h"
#include "byte_stream.h"
#include "text_records.h"

extern char **environ;

namespace {

const char *USAGE =
    "./trust4-hip [OPTIONS]:\n"
    "Required:\n"
    "\t-f STRING: fasta file containing the receptor genome sequence\n"
    "\t-u STRING: path to single-end read file\n"
    "\t\tor\n"
    "\t-1 STRING -2 STRING: path to paried-end read files\n"
    "Optional:\n"
    "\t-o STRING: prefix of the output file (default: trust)\n"
    "\t-c STRING: the path to the kmer count file\n"
    "\t-t INT: number of host threads (default: 1); used by the barcode-mode Add pass (cells are independent)\n"
    "\t-k INT: the starting k-mer size for indexing contigs (default: 9)\n"
    "\t--minHitLen INT: the minimal hit length for a valid overlap (default: auto)\n"
    "\t--skipMateExtension: REQUIRED for paired-end input without barcodes: the mate-pair extension of the assemblies\n"
    "\t\t(main.cpp:2047-2312) is not part of this build, _final.out is the raw assembly\n"
    "\t--trimLevel INT: 0: no trim; 1: trim low quality; 2: trim unmatched (default: 1)\n"
    "\t--cgeneEnd INT: skipping reads mapped to C gene coordinate greater than INT (default: 200)\n"
    "\t--barcode STRING: the path to the barcode file (default: not used)\n"
    "\t--UMI STRING: the path to the UMI file (default: not used)\n"
    "\t--keepNoBarcode: assemble the reads with missing barcodes. (default: ignore the reads)\n"
    "\t--contigMinCov INT: ignore contigs that have bases covered by fewer than INT reads (default: 0)\n"
    "Extension (multi-GPU, see trust4_amd/stage1_dist.py):\n"
    "\t--cellShard R/N: barcode mode only; assemble the R-th of N contiguous ranges of cells, write shard outputs\n"
    "\t--rcclId FILE: with --cellShard, one process per GPU: gather the shards over RCCL (rank 0 creates FILE, the communicator id) and write the merged -o files\n"
    "\t--gatherDir DIR: the same exchange through files in DIR (a directory every rank sees) instead of RCCL\n"
    "\t                 (with either transport a rank builds, processes and counts the read pairs of its own cells only -- the cells follow from the\n"
    "\t                 barcode file -- and the ranks' 21-mer counts are put together in one exchange; --lateShard keeps every read on every rank\n"
    "\t                 up to the cell pass, as a run does by itself when identical reads lie either side of a rank boundary)\n"
    "\t--readShard R/N: one sample over N processes (one per GPU): the rough annotation of the R-th range of the distinct reads here, the results\n"
    "\t                 all-gathered (--rcclId / --gatherDir); rank 0 runs the ordered assembly pass and writes the files, the others end after the exchange\n"
    "\t--allowRawFinal: bulk paired-end input without --skipMateExtension: write the raw assembly as _final.out (the mate-pair extension is not part of this build; logged)\n";

void PrintLog(const char *fmt, ...) {
  char buf[2048], stime[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  time_t t = time(NULL);
  strftime(stime, sizeof stime, "%c", localtime(&t));
  fprintf(stderr, "[%s] %s\n", stime, buf);
}

using namespace t4host;   // nucNum, revCompInPlace, isMateOverlap, SortRead, isLowComplexity, processRead (process_read.h)

// ---- canonical 21-mer counts (KmerCount.hpp) ---------------------------------------------------------
// fn(i) for i in [0, n) on up to `threads` host threads (dynamic chunks); fn must only touch data owned by item i
template <class F> void parallelFor(long long n, int threads, F fn) {
  if (threads <= 1 || n <= 1) { for (long long i = 0; i < n; ++i) fn(i); return; }
  if (threads > n) threads = (int)n;
  std::atomic<long long> next(0);
  const long long chunk = n / (threads * 16LL) > 0 ? n / (threads * 16LL) : 1;
  auto body = [&]() { for (;;) { long long b = next.fetch_add(chunk); if (b >= n) break; long long e = b + chunk < n ? b + chunk : n; for (long long i = b; i < e; ++i) fn(i); } };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; ++t) pool.emplace_back(body);
  body();
  for (auto &th : pool) th.join();
}

struct KmerCounter {
  int k;
  // counts of canonical k-mers, split by a hash of the k-mer so that every shard can be filled by its own thread
  std::vector<std::unordered_map<uint64_t, int>> shards;
  int maxReadLen = -1;
  explicit KmerCounter(int kl, int nShards = 1) : k(kl), shards(nShards > 0 ? nShards : 1) {}
  static uint64_t mix(uint64_t z) { z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
  size_t shardOf(uint64_t kc) const { return shards.size() == 1 ? 0 : (size_t)(mix(kc) % shards.size()); }
  template <class F> void eachValid(const std::string &r, F f) const {
    const int len = (int)r.size();
    const uint64_t mask = k < 32 ? ((1ull << (2 * k)) - 1ull) : ~0ull;
    uint64_t code = 0, rc = 0;
    const int hi = 2 * (k - 1);
    int invalidPos = -1;
    for (int i = 0; i < len; ++i) {
      if (invalidPos != -1) ++invalidPos;
      const uint64_t b = (uint64_t)(nucNum(r[i]) & 3);
      code = ((code << 2) & mask) | b;
      rc = (rc >> 2) | ((3ull - b) << hi);
      if (r[i] == 'N') invalidPos = 0;
      if (invalidPos >= k) invalidPos = -1;
      if (i < k - 1 || invalidPos != -1) continue;
      f(rc < code ? rc : code);
    }
  }
  void addCount(const std::string &r) {   // KmerCount::AddCount (KmerCount.hpp:64-97)
    if ((int)r.size() < k) return;
    eachValid(r, [&](uint64_t kc) { ++shards[shardOf(kc)][kc]; });
  }
  // the same counts for a whole read set, shard s filled by one thread
  template <class GetRead> void addCountAll(long long nReads, int threads, GetRead getRead) {
    const int S = (int)shards.size();
    parallelFor(S, threads < S ? threads : S, [&](long long s) {
      auto &m = shards[(size_t)s];
      for (long long i = 0; i < nReads; ++i) {
        const std::string &r = getRead(i);
        if ((int)r.size() < k) continue;
        eachValid(r, [&](uint64_t kc) { if (S == 1 || (long long)(mix(kc) % (uint64_t)S) == s) ++m[kc]; });
      }
    });
  }
  // KmerCount::AddCountFromFile (KmerCount.hpp:99-120): records ">COUNT\nKMER"; counts <= 1 are skipped, the k-mer is keyed by its
  // code as written (not made canonical), a later record overwrites an earlier one
  bool addCountFromFile(const char *file) {
    FILE *fp = fopen(file, "r");
    if (!fp) return false;
    char tok[100];
    const uint64_t mask = k < 32 ? ((1ull << (2 * k)) - 1ull) : ~0ull;
    while (fscanf(fp, "%99s", tok) != EOF) {
      const int c = atoi(tok + 1);
      if (fscanf(fp, "%99s", tok) == EOF) break;
      if (c <= 1) continue;
      uint64_t code = 0;
      for (int i = 0; tok[i]; ++i) code = ((code << 2) & mask) | (uint64_t)(tok[i] == 'N' ? 0 : (nucNum(tok[i]) & 3));
      shards[shardOf(code)][code] = c;
    }
    fclose(fp);
    return true;
  }
  int count(uint64_t kc) const { const auto &m = shards[shardOf(kc)]; auto it = m.find(kc); return it == m.end() ? 0 : it->second; }
  // GetCountStatsAndTrim (KmerCount.hpp:177-288); read/qual are trimmed in place. qual == nullptr: no trimming.
  void statsAndTrim(std::string &read, std::string *qual, int &minCount, int &medianCount, float &avgCount) const {
    if (maxReadLen == -1) return;
    static thread_local std::vector<int> c;
    if ((int)c.size() < maxReadLen + 1) c.assign(maxReadLen + 1, 0);
    const int len = (int)read.size();
    if (len < k) { minCount = medianCount = -1; avgCount = -1; return; }
    int n = 0, sum = 0;
    eachValid(read, [&](uint64_t kc) {
      int v = count(kc);
      if (v <= 0) v = 1;
      c[n++] = v; sum += v;
    });
    if (n == 0) { minCount = medianCount = -len; avgCount = (float)-len; if (qual) read.clear(); return; }
    const std::string orig = read;   // the reference truncates with a NUL but keeps scanning the old buffer below
    int nul0 = -1, nul1 = -1;
    if (qual) {
      int i;
      for (i = n - 1; i >= 0; --i) if (c[i] > 1) break;
      ++i;
      int badCnt = 0, trimStart = -1;
      for (int j = len - 1; j >= i + k - 1; --j)
        if ((*qual)[j] - 32 <= 15) { ++badCnt; if (badCnt >= 0.1 * (len - j)) trimStart = j; }
      if (trimStart > 0) { n = trimStart - k + 1; read.resize(trimStart); qual->resize(trimStart); nul0 = trimStart; }
      if (trimStart > 0 && trimStart < k) { n = 0; read.clear(); qual->clear(); nul1 = 0; }
    }
    if (n > 0) std::sort(c.begin(), c.begin() + n);
    minCount = c[0]; medianCount = c[n > 0 ? n / 2 : 0]; avgCount = (float)(sum / (double)n);
    for (int i = 0; i < len; ++i)
      if (i != nul0 && i != nul1 && orig[i] == 'N') { if (minCount >= 0) minCount = 0; else if (minCount <= 0) --minCount; }
  }
};

bool compReadWithBarcode(const SortRead &a, const SortRead &b) {   // main.cpp:128-136
  if (a.barcode != -1 && a.barcode != b.barcode) return a.barcode < b.barcode;
  if (a.barcode != -1 && b.barcode != -1 && a.barcodeMinCnt != b.barcodeMinCnt) return a.barcodeMinCnt > b.barcodeMinCnt;
  return a < b;
}

// std::sort(v.begin(), v.end(), less) on the host threads. The reference sorts with std::sort, whose result is only defined by the
// comparator when no two elements tie: the read list is sorted as a permutation on the threads, and only if no two neighbours of the result tie -- the order is then THE sorted order, whatever algorithm produced it --
// is the permutation applied. With a tie (or when the caller knows the comparator is not a strict weak order for its input) the
// list goes through std::sort itself, as before.
// `spare`: a list of the same size from an earlier call (its storage takes the sorted records; it comes back holding the old storage)
template <class Less> void sortReadsOnThreads(std::vector<SortRead> &v, int threads, Less less, bool orderIsStrict = true, std::vector<SortRead> *spare = nullptr) {
  const size_t n = v.size();
  const size_t minN = getenv("T4_SORT_MIN") ? (size_t)atoll(getenv("T4_SORT_MIN")) : 65536;   // testing aid: small inputs through the threaded path
  const size_t minChunk = minN / 64 > 8 ? minN / 64 : 8;
  if (threads <= 1 || n < minN || n < 2 * minChunk || !orderIsStrict) { std::sort(v.begin(), v.end(), less); return; }
  // sample sort of the permutation: splitters from a sorted sample, every element classified against them (a binary search), the
  // buckets sorted side by side -- no serial merge at the end
  int parts = 1;
  while (parts < 2 * threads) parts *= 2;
  if (parts > 256) parts = 256;   // (bucket numbers are kept in bytes)
  while (parts > 1 && (size_t)parts * minChunk > n) parts /= 2;
  auto byRead = [&](uint32_t a, uint32_t b) { return less(v[a], v[b]); };
  std::vector<uint32_t> sample;
  { const size_t want = (size_t)parts * 48 < n ? (size_t)parts * 48 : n; for (size_t i = 0; i < want; ++i) sample.push_back((uint32_t)(n * i / want)); }
  std::sort(sample.begin(), sample.end(), byRead);
  std::vector<uint32_t> split;
  for (int p = 1; p < parts; ++p) split.push_back(sample[sample.size() * (size_t)p / (size_t)parts]);
  const int slices = threads * 4;
  auto sliceAt = [&](int i) { return n * (size_t)i / (size_t)slices; };
  std::vector<unsigned char> bucketOf(n);
  std::vector<size_t> counts((size_t)slices * parts, 0);
  parallelFor(slices, threads, [&](long long sl) {
    size_t *cnt = &counts[(size_t)sl * parts];
    for (size_t i = sliceAt((int)sl); i < sliceAt((int)sl + 1); ++i) {
      int lo = 0, hi = (int)split.size();   // bucket = number of splitters that are less than the element
      while (lo < hi) { const int mid = (lo + hi) / 2; if (less(v[split[(size_t)mid]], v[i])) lo = mid + 1; else hi = mid; }
      bucketOf[i] = (unsigned char)lo; ++cnt[lo];
    }
  });
  std::vector<size_t> bucketStart((size_t)parts + 1, 0);
  for (int p = 0; p < parts; ++p) { size_t c = 0; for (int sl = 0; sl < slices; ++sl) c += counts[(size_t)sl * parts + p]; bucketStart[(size_t)p + 1] = bucketStart[(size_t)p] + c; }
  { std::vector<size_t> run(bucketStart.begin(), bucketStart.end() - 1);   // where each slice writes inside each bucket
    for (int sl = 0; sl < slices; ++sl) for (int p = 0; p < parts; ++p) { const size_t c = counts[(size_t)sl * parts + p]; counts[(size_t)sl * parts + p] = run[(size_t)p]; run[(size_t)p] += c; } }
  std::vector<uint32_t> perm(n);
  parallelFor(slices, threads, [&](long long sl) {
    size_t *at = &counts[(size_t)sl * parts];
    for (size_t i = sliceAt((int)sl); i < sliceAt((int)sl + 1); ++i) perm[at[bucketOf[i]]++] = (uint32_t)i;
  });
  parallelFor(parts, threads, [&](long long p) { std::sort(perm.begin() + bucketStart[(size_t)p], perm.begin() + bucketStart[(size_t)p + 1], byRead); });
  const uint32_t *src = perm.data();
  std::atomic<bool> tie(false);
  parallelFor((long long)n - 1, threads, [&](long long i) { if (!less(v[src[i]], v[src[i + 1]])) tie.store(true, std::memory_order_relaxed); });
  if (tie.load()) {
    if (getenv("T4_TIMING")) fprintf(stderr, "timing: two reads of the list tie under the comparator: sorted by std::sort as in the reference\n");
    std::sort(v.begin(), v.end(), less);
    return;
  }
  std::vector<SortRead> fresh;
  std::vector<SortRead> &out = spare ? *spare : fresh;
  out.resize(n);   // (2 M records of 312 bytes: built once; the second sort of a run finds them in `spare`)
  parallelFor((long long)n, threads, [&](long long i) { out[(size_t)i] = std::move(v[src[i]]); });
  v.swap(out);
}

// SeqSet::DnaToAa / HasMotif (SeqSet.hpp:638-749, 5029-5074); note that the reference translates `read`, not its
// reverse complement, whatever the strand
char dnaToAa(char a, char b, char c) {
  if (a == 'N' || b == 'N' || c == 'N' || a == 'M' || b == 'M' || c == 'M') return '?';
  const bool cAG = (c == 'A' || c == 'G');
  if (a == 'A') {
    if (b == 'A') return cAG ? 'K' : 'N';
    if (b == 'C') return 'T';
    if (b == 'G') return cAG ? 'R' : 'S';
    return c == 'G' ? 'M' : 'I';
  } else if (a == 'C') {
    if (b == 'A') return cAG ? 'Q' : 'H';
    if (b == 'C') return 'P';
    if (b == 'G') return 'R';
    return 'L';
  } else if (a == 'G') {
    if (b == 'A') return cAG ? 'E' : 'D';
    if (b == 'C') return 'A';
    if (b == 'G') return 'G';
    return 'V';
  }
  if (b == 'A') return cAG ? '_' : 'Y';
  if (b == 'C') return 'S';
  if (b == 'G') return c == 'A' ? '_' : c == 'G' ? 'W' : 'C';
  return cAG ? 'L' : 'F';
}
int hasMotif(const std::string &read, int strand) {
  if (strand == 0) return 0;
  const int len = (int)read.size();
  std::string aa(len + 1, '\0');
  int ret = 0;
  for (int k = 0; k <= 2; ++k) {
    int j = 0;
    for (int i = k; i + 2 < len; i += 3, ++j) aa[j] = dnaToAa(read[i], read[i + 1], read[i + 2]);
    for (int i = 0; i + 2 < j; ++i) if (aa[i] == 'Y' && aa[i + 1] == 'Y' && aa[i + 2] == 'C') { ret |= 2; break; }
    for (int i = 0; i + 3 < j; ++i) if ((aa[i] == 'F' || aa[i] == 'W') && aa[i + 1] == 'G' && aa[i + 3] == 'G') { ret |= 1; break; }
  }
  return ret;
}

// The end of a run whose files are written and closed: the process leaves without walking its heaps (millions of read records, the
// host replica, the device arenas -- 1.3 s of a 14 s barcode-mode run); the driver and the OS reclaim them. T4_FULL_TEARDOWN=1 keeps
// the orderly destruction (leak checkers, the emulator build's tests of it).
void leave(int status) {
  if (getenv("T4_FULL_TEARDOWN") || getenv("T4_PHASE_DUMP")) return;   // (the phase dump of a T4_PHASE_TIMING build is written by t4_destroy)
  exit(status);   // (exit, not _exit: stdio is flushed and atexit handlers run -- rocprofv3 writes its traces there)
}
thread_local t4_ctx *tlsErrCtx = nullptr;   // the ctx whose errors this thread reports (a cell group's own; else the caller's)
void die(t4_ctx *ctx, const char *what, int rc) {
  if (tlsErrCtx) ctx = tlsErrCtx;
  fprintf(stderr, "%s failed (%d): %s\n", what, rc, ctx ? t4_last_error(ctx) : "");
  exit(EXIT_FAILURE);
}

}  // namespace

int main(int argc, char *argv[]) {
  if (argc <= 1) { fprintf(stderr, "%s", USAGE); return 0; }
  static struct option long_options[] = {{"trimLevel", required_argument, 0, 10001}, {"skipMateExtension", no_argument, 0, 10005},
                                         {"minHitLen", required_argument, 0, 10006}, {"cgeneEnd", required_argument, 0, 10008},
                                         {"barcode", required_argument, 0, 10002}, {"UMI", required_argument, 0, 10004},
                                         {"keepNoBarcode", no_argument, 0, 10003}, {"contigMinCov", required_argument, 0, 10007},
                                         {"cellShard", required_argument, 0, 10100}, {"rcclId", required_argument, 0, 10101}, {"gatherDir", required_argument, 0, 10102}, {"readShard", required_argument, 0, 10103}, {"lateShard", no_argument, 0, 10104}, {"allowRawFinal", no_argument, 0, 10105}, {"debug-ns", required_argument, 0, 10000},
                                         {(char *)0, 0, 0, 0}};
  int indexKmerLength = 9, changeKmerLengthThreshold = 4096, trimLevel = 1, minHitLen = -1, constantGeneEnd = 200;
  int shardRank = 0, shardCount = 1, threadCnt = 1, contigMinCov = 0;
  bool annotSharded = false;
  bool allowRawFinal = false;   // --allowRawFinal: bulk paired-end input without --skipMateExtension writes the raw assembly as _final.out (logged)
  bool lateShard = false;   // --lateShard (set by the fallback of the early shard, see below): every rank runs the phases before the cell pass over ALL reads, as round 3 did
  int annotRank = 0, annotCount = 1;   // --readShard R/N: the read-only pass of ONE sample (rough annotation) by read range over N processes, results all-gathered; rank 0 goes on alone
  std::string gatherDir;    // --gatherDir DIR: the same exchange through files of a directory every rank sees (tests without RCCL)
  std::string rcclIdPath;   // --rcclId FILE: the shards' results are gathered inside the engine (t4_comm: RCCL), rank 0 writes the merged files
  bool keepMissingBarcode = false, skipMateExtension = false;
  std::string refFa, outputPrefix = "trust", kmerCountFile;
  struct NovelFa { std::string file; int kmerLength; };
  std::vector<NovelFa> novelFa;   // --debug-ns: contigs put into the set before any read (main.cpp:709-712)
  ThreadedSeqReader reads, mateReads, barcodeFile, umiFile;   // each file is read and split on its own thread
  bool hasMate = false, hasBarcode = false, hasUmi = false;
  int c, oi = 0;
  while ((c = getopt_long(argc, argv, "f:u:1:2:o:c:t:k:", long_options, &oi)) != -1) {
    if (c == 'f') refFa = optarg;
    else if (c == 'u') reads.files.push_back(optarg);
    else if (c == '1') { reads.files.push_back(optarg); hasMate = true; }
    else if (c == '2') { mateReads.files.push_back(optarg); hasMate = true; }
    else if (c == 'o') outputPrefix = optarg;
    else if (c == 't') threadCnt = atoi(optarg) > 0 ? atoi(optarg) : 1;
    else if (c == 'k') indexKmerLength = atoi(optarg);
    else if (c == 'c') kmerCountFile = optarg;
    else if (c == 10000) novelFa.push_back(NovelFa{optarg, indexKmerLength});
    else if (c == 10001) trimLevel = atoi(optarg);
    else if (c == 10005) skipMateExtension = true;
    else if (c == 10006) minHitLen = atoi(optarg);
    else if (c == 10008) constantGeneEnd = atoi(optarg);
    else if (c == 10002) { barcodeFile.files.push_back(optarg); hasBarcode = true; }
    else if (c == 10004) { umiFile.files.push_back(optarg); hasUmi = true; }
    else if (c == 10101) rcclIdPath = optarg;
    else if (c == 10102) gatherDir = optarg;
    else if (c == 10104) lateShard = true;
    else if (c == 10103) { if (sscanf(optarg, "%d/%d", &annotRank, &annotCount) != 2 || annotCount < 1 || annotRank < 0 || annotRank >= annotCount) { fprintf(stderr, "--readShard takes R/N with 0 <= R < N\n"); return EXIT_FAILURE; } annotSharded = true; }
    else if (c == 10100) { if (sscanf(optarg, "%d/%d", &shardRank, &shardCount) != 2 || shardCount < 1 || shardRank < 0 || shardRank >= shardCount) { fprintf(stderr, "--cellShard takes R/N with 0 <= R < N\n"); return EXIT_FAILURE; } }
    else if (c == 10105) allowRawFinal = true;
    else if (c == 10003) keepMissingBarcode = true;
    else if (c == 10007) contigMinCov = atoi(optarg);
    else { fprintf(stderr, "%s", USAGE); return EXIT_FAILURE; }
  }
  if (refFa.empty()) { fprintf(stderr, "Need to use -f to specify the receptor genome sequence.\n"); return EXIT_FAILURE; }
  if (hasMate && !hasBarcode && !skipMateExtension && !allowRawFinal) {
    // main.cpp:2018-2312: the reference would go on to its mate-pair extension (ExtendSeqFromReads, RemoveRedundantSeq) and the
    // annotator reads _final.out. A silent copy of the raw assembly there would change contigs and CDR3 calls downstream.
    fprintf(stderr, "trust4-hip: the mate-pair extension of the assemblies (what the reference runs for paired-end input without barcodes) is not part of this build.\n"
                    "Pass --skipMateExtension (run-trust4 forwards it; _final.out is then the raw assembly, as in the reference), or --allowRawFinal to get that file knowingly without the flag.\n");
    return EXIT_FAILURE;
  }
  if (getenv("T4_THREADS")) threadCnt = atoi(getenv("T4_THREADS")) > 0 ? atoi(getenv("T4_THREADS")) : 1;
  // Switches that exist for the CPU suite's negative controls and forced fall-backs only. They are compiled into the emulator build of
  // the driver (-DT4_TEST_KNOBS, tests/test_stage1_e2e.py:_emulated_driver) and into nothing that ships: one of them changes the result.
#ifdef T4_TEST_KNOBS
  const bool testNoCountMerge = getenv("T4_TEST_NO_COUNT_MERGE") != nullptr;   // the other ranks' 21-mer counts are NOT added (the files must then differ)
  const bool testForceCoupled = getenv("T4_TEST_FORCE_COUPLED") != nullptr;    // the early shard's fall-back on inputs that do not need it
#else
  const bool testNoCountMerge = false, testForceCoupled = false;
#endif
  if (shardCount > 1 && (!hasBarcode || keepMissingBarcode)) { fprintf(stderr, "--cellShard needs --barcode: without barcodes the Add pass does not shard (DESIGN.md 6).\n"); return EXIT_FAILURE; }
  if (annotSharded && shardCount > 1) { fprintf(stderr, "--readShard and --cellShard are two ways to spread one sample: take one.\n"); return EXIT_FAILURE; }
  if (annotSharded && rcclIdPath.empty() && gatherDir.empty()) { fprintf(stderr, "--readShard needs --rcclId FILE or --gatherDir DIR for the exchange of the annotations.\n"); return EXIT_FAILURE; }

  // The device, its runtime and the reference set come up on their own thread while the reads are parsed, merged and counted
  // (nothing before the rough annotation touches the GPU); gpuReady() joins it and reports its errors as the serial code did.
  t4_ctx *ctx = nullptr;
  t4_index *refSet = nullptr;
  int rc = 0, initRc = 0;
  const char *initWhat = nullptr;
  std::thread initThread([&]() {
    if ((initRc = t4_init(getenv("T4_DEVICE") ? atoi(getenv("T4_DEVICE")) : 0, &ctx))) { initWhat = "t4_init"; return; }
    if ((initRc = t4_index_create(ctx, trimLevel > 1 ? 7 : 9, 0, &refSet))) { initWhat = "t4_index_create"; return; }
    if ((initRc = t4_index_set_params(refSet, 17, trimLevel > 1 ? 0 : 10, 0.9))) { initWhat = "t4_index_set_params"; return; }
    if ((initRc = t4_index_load_ref_fasta(refSet, refFa.c_str()))) { initWhat = "t4_index_load_ref_fasta"; return; }
    if (t4_index_size(refSet) == 0) return;
    if ((initRc = t4_index_commit(refSet))) initWhat = "t4_index_commit";
  });
  auto gpuReady = [&]() {
    if (!initThread.joinable()) return;
    const auto tw = std::chrono::steady_clock::now();
    initThread.join();
    if (getenv("T4_TIMING")) PrintLog("timing: waited %.2f s for the device and the reference set (they come up on their own thread from the start)", std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count());
    if (initRc && !ctx) { fprintf(stderr, "trust4-hip needs an MI355X (t4_init failed: %d); there is no CPU path.\n", initRc); exit(EXIT_FAILURE); }
    if (initRc) die(ctx, initWhat, initRc);
    if (t4_index_size(refSet) == 0) { fprintf(stderr, "Need to use -f to specify the receptor genome sequence.\n"); exit(EXIT_FAILURE); }
  };
  // ---- the transport of the sharded modes (--cellShard): RCCL over xGMI (--rcclId: t4_comm on the ctx's stream) or files in a directory
  // every rank sees (--gatherDir: the CPU tests). After the fallback of the early shard (--lateShard) the names carry a tag of their own,
  // so that nothing of the first attempt is taken for the second's.
  t4_comm *comm = nullptr;
  int exchangeNo = 0;
  const std::string xferTag = lateShard ? "retry." : "";
  auto fileOf = [&](int no, int r) { return gatherDir + "/" + xferTag + "x" + std::to_string(no) + ".rank" + std::to_string(r); };
  auto readWhole = [](const std::string &path, std::string &out) { FILE *fp = fopen(path.c_str(), "rb"); if (!fp) return false; char buf[1 << 16]; size_t n; out.clear(); while ((n = fread(buf, 1, sizeof buf, fp)) > 0) out.append(buf, n); fclose(fp); return true; };
  // The communicator of --rcclId, brought up so that the FIRST multi-GPU run fails soft (RCCL never ran with more than
  // one rank on any machine the builder had): t4_comm_init checks itself (a 1-int all-gather must return the rank numbers), every
  // rank then publishes how its communicator came up (FILE.status.rank<r>) and reads everybody's; unless every rank says "ok" ALL
  // ranks give their communicator up and run the same exchange through files in FILE.files/ (a directory beside the id file: node-
  // local, as the id file is). The decision is the same on every rank, it is logged, and it is reported in the statistics JSON.
  std::string transportNote = gatherDir.empty() ? (rcclIdPath.empty() ? "none" : "RCCL") : "files";
  auto commUp = [&](int rank, int count, const std::string &idPath) -> bool {   // true: RCCL is up; false: the file transport is on (gatherDir set)
    gpuReady();
    auto statusOf = [&](int r) { return idPath + ".status.rank" + std::to_string(r); };
    //  A status file an earlier run left on the same path must not be taken for this run's: a rank removes its own before
    // its communicator comes up -- no rank gets through the self-check of t4_comm_init before every rank is inside it, so by the time
    // a rank that came up reads the others' files, theirs are this run's or absent --, and every status carries the run's nonce (the
    // first bytes of the id file rank 0 made for THIS run); a file with another nonce counts as not written yet. A rank that could not
    // even read the id writes "-": it has failed, which sends every rank to the file transport whatever the others say.
    (void)unlink(statusOf(rank).c_str());
    const int irc = t4_comm_init(ctx, rank, count, idPath.c_str(), &comm);
    std::string nonce = "-";
    {
      std::string idBytes;
      if (readWhole(idPath, idBytes) && !idBytes.empty()) {
        static const char *hx = "0123456789abcdef";
        nonce.clear();
        for (size_t t = 0; t < idBytes.size() && t < 16; ++t) { nonce.push_back(hx[((unsigned char)idBytes[t]) >> 4]); nonce.push_back(hx[((unsigned char)idBytes[t]) & 15]); }
      }
    }
    const std::string why = nonce + ":" + (irc ? (std::string("fail ") + t4_last_error(ctx)) : std::string("ok"));
    {
      FILE *fp = fopen((statusOf(rank) + ".tmp").c_str(), "wb");
      if (!fp || fwrite(why.data(), 1, why.size(), fp) != why.size()) { if (fp) fclose(fp); die(ctx, "t4_comm_init (status file)", irc ? irc : T4_ERR_IO); }
      fclose(fp);
      if (rename((statusOf(rank) + ".tmp").c_str(), statusOf(rank).c_str())) die(ctx, "t4_comm_init (status file)", irc ? irc : T4_ERR_IO);
    }
    bool allOk = true; std::string firstBad;
    for (int r = 0; r < count; ++r) {
      std::string st; bool got1 = false;
      // (the bound of exchangeFiles: with the input dealt out by cells the ranks reach their first exchange minutes apart)
      for (int tries = 0; tries < 36000 && !got1; ++tries) {
        got1 = readWhole(statusOf(r), st) && !st.empty() && (st.compare(0, nonce.size() + 1, nonce + ":") == 0 || st.compare(0, 7, "-:fail ") == 0 || nonce == "-");
        if (!got1) usleep(50000);
      }
      if (!got1) die(ctx, "t4_comm_init (no status from every rank)", irc ? irc : T4_ERR_IO);
      st = st.substr(st.find(':') + 1);
      if (st != "ok") { allOk = false; if (firstBad.empty()) firstBad = "rank " + std::to_string(r) + ": " + st; }
    }
    if (allOk) return true;
    if (comm) { t4_comm_destroy(comm); comm = nullptr; }
    gatherDir = idPath + ".files";
    (void)mkdir(gatherDir.c_str(), 0777);
    transportNote = "files (fallback from RCCL: " + firstBad + ")";
    for (char &ch : transportNote) if (ch == '"' || ch == '\\' || ch == '\n') ch = ' ';
    if (rank == 0) PrintLog("RCCL did not come up on every rank (%s): the exchange runs through files in %s.", firstBad.c_str(), gatherDir.c_str());
    return false;
  };
  auto exchangeFiles = [&](const std::string &mine, bool everyRank, std::vector<std::string> &got, int no) -> bool {
    const std::string tmp = fileOf(no, shardRank) + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "wb");
    if (!fp || fwrite(mine.data(), 1, mine.size(), fp) != mine.size()) { if (fp) fclose(fp); return false; }
    fclose(fp);
    if (rename(tmp.c_str(), fileOf(no, shardRank).c_str())) return false;
    if (!everyRank && shardRank != 0) return true;
    for (int r = 0; r < shardCount; ++r) {
      bool ok = false;
      for (int tries = 0; tries < 36000 && !ok; ++tries) { ok = readWhole(fileOf(no, r), got[(size_t)r]); if (!ok) usleep(50000); }
      if (!ok) return false;
    }
    return true;
  };
  const auto &exchangeRef = exchangeFiles;
  // every rank contributes `mine`; everyRank: all ranks receive all contributions, else only rank 0 does
  auto exchange = [&](const std::string &mine, bool everyRank, std::vector<std::string> &got) -> bool {
    got.assign((size_t)shardCount, std::string());
    const int no = exchangeNo++;
    if (!gatherDir.empty()) return exchangeFiles(mine, everyRank, got, no);
    if (!comm && !commUp(shardRank, shardCount, rcclIdPath + (lateShard ? ".retry" : ""))) return exchangeRef(mine, everyRank, got, no);   // (fell back to files)
    void *all = nullptr;
    std::vector<int64_t> sizes((size_t)shardCount);
    const int rr = everyRank ? t4_comm_allgather_bytes(comm, mine.data(), (int64_t)mine.size(), &all, sizes.data())
                             : t4_comm_gather_bytes(comm, mine.data(), (int64_t)mine.size(), 0, &all, sizes.data());
    if (rr) die(ctx, everyRank ? "t4_comm_allgather_bytes" : "t4_comm_gather_bytes", rr);
    if (all) {
      size_t at = 0;
      for (int r = 0; r < shardCount; ++r) { got[(size_t)r].assign((const char *)all + at, (size_t)sizes[(size_t)r]); at += (size_t)sizes[(size_t)r]; }
      free(all);
    }
    return true;
  };
  PrintLog("Start to assemble reads.");
  // wall-clock marks of the phases (written to $T4_STATS_JSON for bench.py)
  const auto tStart = std::chrono::steady_clock::now();
  std::vector<std::pair<std::string, double>> phaseMarks;
  auto mark = [&](const char *name) { phaseMarks.push_back({name, std::chrono::duration<double>(std::chrono::steady_clock::now() - tStart).count()}); };
  double annotKernelMs = 0; long long annotHits = 0, annotReads = 0;

  // ---- read input, mate processing, 21-mer counting (main.cpp:787-915)
  KmerCounter kmerCount(21, threadCnt);
  std::vector<SortRead> sortedReads;
  struct InPair { SortRead a, b; bool haveMate; };
  std::vector<InPair> block;
  const size_t BLOCK = 262144;
  double secProcess = 0, secMerge = 0;
  std::vector<std::vector<SortRead>> chunkOuts;
  std::vector<SortRead> sortSpare;   // the second list of the threaded sorts
  // T4_GPU_MATEOVERLAP=1 (opt-in this round): the two AlignAlgo::IsMateOverlap tests of every pair of a block come from
  // t4_mate_overlap (one pair per wavefront) instead of the host threads; the merge itself stays on the host.
  const bool gpuMate = getenv("T4_GPU_MATEOVERLAP") && atoi(getenv("T4_GPU_MATEOVERLAP")) != 0;
  const bool gpuProcess = getenv("T4_GPU_PROCESSREAD") && atoi(getenv("T4_GPU_PROCESSREAD")) != 0;
  long long ppKinds[4] = {0, 0, 0, 0}, ppBlocksOnHost = 0;
  // (a block is processed on the host threads WHILE the next one is parsed: processBlock runs on its own thread, one block at a time)
  auto processBlock = [&](std::vector<InPair> &block) {   // ProcessRead of every pair of the block on the host threads, results appended in input order
    auto t0 = std::chrono::steady_clock::now();
    // results per CHUNK of consecutive pairs (one vector per chunk, filled by one thread in input order: a vector per pair was a
    // million small allocations per block, freed across threads)
    const size_t PP_CHUNK = 1024;
    std::vector<std::vector<SortRead>> &outs = chunkOuts;   // (the chunk vectors keep their storage from block to block: no fresh pages after the first)
    if (outs.size() < (block.size() + PP_CHUNK - 1) / PP_CHUNK) outs.resize((block.size() + PP_CHUNK - 1) / PP_CHUNK);
    const size_t nChunks = (block.size() + PP_CHUNK - 1) / PP_CHUNK;
    std::vector<int32_t> pre;
    bool anyMate = false;
    for (const InPair &ip : block) if (ip.haveMate) { anyMate = true; break; }
    if (gpuMate && !gpuProcess && anyMate) {
      gpuReady();
      const int n = (int)block.size();
      std::string fc, sc;
      std::vector<int64_t> fo(1, 0), so(1, 0);
      std::vector<int32_t> mo1((size_t)n), mo2((size_t)n), o1((size_t)n * 3), o2((size_t)n * 3);
      for (int i = 0; i < n; ++i) {
        if (block[(size_t)i].haveMate) {
          std::string rcMate = block[(size_t)i].b.read;
          revCompInPlace(rcMate);
          fc += rcMate; sc += block[(size_t)i].a.read;
        }
        fo.push_back((int64_t)fc.size()); so.push_back((int64_t)sc.size());
        const int tot = block[(size_t)i].haveMate ? (int)(block[(size_t)i].a.read.size() + block[(size_t)i].b.read.size()) : 0;
        mo1[(size_t)i] = tot / 10 > 31 ? 31 : tot / 10; mo2[(size_t)i] = tot / 20 > 31 ? 31 : tot / 20;
      }
      if ((rc = t4_mate_overlap(ctx, n, fo.data(), fc.data(), so.data(), sc.data(), mo1.data(), 0, o1.data()))) die(ctx, "t4_mate_overlap", rc);
      if ((rc = t4_mate_overlap(ctx, n, so.data(), sc.data(), fo.data(), fc.data(), mo2.data(), 1, o2.data()))) die(ctx, "t4_mate_overlap", rc);
      pre.resize((size_t)n * 6);
      for (int i = 0; i < n; ++i) for (int j = 0; j < 3; ++j) { pre[(size_t)i * 6 + j] = o1[(size_t)i * 3 + j]; pre[(size_t)i * 6 + 3 + j] = o2[(size_t)i * 3 + j]; }
    }
    // T4_GPU_PROCESSREAD=1 (opt-in): the whole of ProcessRead for the pairs of the block on the device (t4_process_pairs: both
    // IsMateOverlap tests, the read-through clip / merge / choice of a mate, IsLowComplexity); the host only builds the records
    std::vector<int32_t> meta;
    std::vector<int64_t> ppOut;
    std::string ppR, ppQ;
    if (gpuProcess && anyMate) {
      gpuReady();
      const int n = (int)block.size();
      std::string c1, q1, c2, q2;
      std::vector<int64_t> o1(1, 0), o2(1, 0);
      std::vector<unsigned char> hq((size_t)n, 0);
      ppOut.assign(1, 0);
      bool anyQ1 = false, anyQ2 = false;
      for (const InPair &ip : block) { if (ip.haveMate && ip.a.hasQual) anyQ1 = true; if (ip.haveMate && ip.b.hasQual) anyQ2 = true; }
      for (int i = 0; i < n; ++i) {
        const InPair &ip = block[(size_t)i];
        if (ip.haveMate) {
          c1 += ip.a.read; c2 += ip.b.read;
          if (anyQ1) { if (ip.a.hasQual && ip.a.qual.size() == ip.a.read.size()) q1 += ip.a.qual; else q1.append(ip.a.read.size(), '\0'); }
          if (anyQ2) { if (ip.b.hasQual && ip.b.qual.size() == ip.b.read.size()) q2 += ip.b.qual; else q2.append(ip.b.read.size(), '\0'); }
          hq[(size_t)i] = (unsigned char)((ip.a.hasQual && ip.a.qual.size() == ip.a.read.size() ? 1 : 0) | (ip.b.hasQual && ip.b.qual.size() == ip.b.read.size() ? 2 : 0));
          ppOut.push_back(ppOut.back() + (int64_t)(ip.a.read.size() + ip.b.read.size() + 1));
        } else ppOut.push_back(ppOut.back() + 1);
        o1.push_back((int64_t)c1.size()); o2.push_back((int64_t)c2.size());
      }
      ppR.assign((size_t)ppOut.back() + 1, '\0'); ppQ.assign((size_t)ppOut.back() + 1, '\0');
      meta.assign((size_t)n * 4, 0);
      rc = t4_process_pairs(ctx, n, o1.data(), c1.data(), anyQ1 ? q1.data() : nullptr, o2.data(), c2.data(), anyQ2 ? q2.data() : nullptr, hq.data(),
                            ppOut.data(), &ppR[0], &ppQ[0], meta.data());
      if (rc == T4_ERR_UNSUPPORTED) { meta.clear(); ++ppBlocksOnHost; }   // (a mate beyond the kernel's 384 bp: this block takes the host's ProcessRead, which has no such limit)
      else if (rc) die(ctx, "t4_process_pairs", rc);
      else for (int i = 0; i < n; ++i) if (block[(size_t)i].haveMate) ++ppKinds[meta[(size_t)i * 4] & 3];
    }
    auto onePair = [&](long long i, std::vector<SortRead> &out) {
      const InPair &ip = block[(size_t)i];
      if (!meta.empty() && ip.haveMate) {
        const int len = meta[(size_t)i * 4 + 1], fl = meta[(size_t)i * 4 + 2];
        if (fl & 1) {
          SortRead r1 = ip.a;
          if (fl & 16) {
            r1.read.assign(ppR, (size_t)ppOut[(size_t)i], (size_t)len);
            if (fl & 8) r1.qual.assign(ppQ, (size_t)ppOut[(size_t)i], (size_t)len);
          }
          r1.hasQual = (fl & 8) != 0;
          out.push_back(r1);
          if (fl & 4) { SortRead w = r1; w.id += ".1"; out.push_back(w); }
        }
        if (fl & 2) {
          SortRead r2 = ip.b;
          for (char &ch : r2.read) if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' && ch != 'N') ch = 'N';   // what two reverse complements leave
          out.push_back(r2);
        }
        return;
      }
      processRead(ip.a, ip.b, ip.haveMate, out, pre.empty() ? nullptr : &pre[(size_t)i * 6]);
    };
    parallelFor((long long)nChunks, threadCnt, [&](long long c) {
      std::vector<SortRead> &out = outs[(size_t)c];
      const size_t lo = (size_t)c * PP_CHUNK, hi = lo + PP_CHUNK < block.size() ? lo + PP_CHUNK : block.size();
      out.clear();
      out.reserve((hi - lo) * 2 + 2);
      for (size_t i = lo; i < hi; ++i) onePair((long long)i, out);
    });
    auto t1 = std::chrono::steady_clock::now();
    {   // the chunks at their places in the read list, moved on the threads (the list has room for the whole input when its size could
        // be told from the first block and the file's size: no reallocation, every page of it touched once)
      std::vector<size_t> first(nChunks + 1, sortedReads.size());
      for (size_t c = 0; c < nChunks; ++c) first[c + 1] = first[c] + outs[c].size();
      sortedReads.resize(first[nChunks]);
      parallelFor((long long)nChunks, threadCnt, [&](long long c) {
        std::vector<SortRead> &v = outs[(size_t)c];
        for (size_t j = 0; j < v.size(); ++j) sortedReads[first[(size_t)c] + j] = std::move(v[j]);
        v.clear();
      });
    }
    secProcess += std::chrono::duration<double>(t1 - t0).count();
    secMerge += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  };
  // The readers deliver whole blocks of records; the only serial work per record is the numbering of barcodes and UMIs in order of
  // first appearance (main.cpp:799-842). Everything else -- building the read records, ProcessRead -- runs on the host threads, one
  // batch of blocks at a time, while the next batch is read.
  struct Unit { ThreadedSeqReader::Block r, m; std::vector<int> bc, umi; std::vector<char> skip; };
  std::vector<Unit> units, inProcess;
  size_t unitPairs = 0;
  std::thread processThread;
  double secWaitProcess = 0;
  const auto tInput0 = std::chrono::steady_clock::now();
  auto flushBlock = [&]() {
    { const auto tw = std::chrono::steady_clock::now(); if (processThread.joinable()) processThread.join(); secWaitProcess += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count(); }
    for (Unit &u : inProcess) { reads.recycle(u.r); mateReads.recycle(u.m); }   // the consumed blocks go back to their readers, strings and all
    inProcess.clear();
    inProcess.swap(units);
    unitPairs = 0;
    if (inProcess.empty()) return;
    processThread = std::thread([&]() {
      std::vector<std::pair<uint32_t, uint32_t>> at;
      for (size_t u = 0; u < inProcess.size(); ++u) for (size_t i = 0; i < inProcess[u].r.size(); ++i) if (!inProcess[u].skip[i]) at.push_back({(uint32_t)u, (uint32_t)i});
      block.resize(at.size());   // (not cleared: the strings of the pairs before are swapped into the records below and travel back to the readers)
      parallelFor((long long)at.size(), threadCnt, [&](long long k) {
        Unit &un = inProcess[at[(size_t)k].first];
        const size_t i = at[(size_t)k].second;
        InPair &ip = block[(size_t)k];
        ThreadedSeqReader::Rec &r = un.r[i];
        ip.a.id.swap(r.id); ip.a.read.swap(r.seq); ip.a.qual.swap(r.qual); ip.a.hasQual = r.hasQual;
        ip.a.barcode = ip.b.barcode = un.bc[i]; ip.a.umi = ip.b.umi = un.umi[i];
        ip.haveMate = !un.m.empty();
        if (ip.haveMate) { ThreadedSeqReader::Rec &m = un.m[i]; ip.b.id.swap(m.id); ip.b.read.swap(m.seq); ip.b.qual.swap(m.qual); ip.b.hasQual = m.hasQual; }
      });
      processBlock(block);
    });
  };
  int firstReadLen = -1, nIn = 0;
  bool reservedReadList = false;
  StrNumbering barcodeNumbers, umiNumbers;   // strings -> dense ints in order of first appearance (main.cpp:812-820, 831-842)
  // ---- --cellShard R/N with a transport: the INPUT is dealt out by cells (round 5; VERDICT r3 / r4 "parse / ProcessRead / counts
  // replicated"). Which cells are a rank's follows from the barcode file alone -- barcodes are numbered in order of first appearance
  // (main.cpp:812-820) and the ranks get contiguous ranges of those numbers with about the same number of read pairs --, so every
  // rank reads the barcode file once ahead of the input loop, and the loop then builds, ProcessReads and counts the 21-mers of the
  // pairs of ITS cells only. Every rank still splits the FASTQ text of the whole sample into records (no record can be found without
  // the ones before it) and numbers every UMI (numbers are in order of first appearance over the whole sample, main.cpp:831-842).
  // (Under T4_GPU_PARSE=1 the device splits the text, and the rank's host threads touch the records of its own cells only: below.)
  // The 21-mer counts of the whole sample, which the statistics of every read look at, are put together afterwards: counts only
  // ever add up (KmerCount.hpp:64-97), so every rank hands the others the pairs of its table and adds theirs where it holds the k-mer
  // (t4_kmer_count_export / _merge; one all-gather). T4_SHARD_INPUT=0: every rank runs the input phases over the whole sample
  // and lets go of the other ranks' reads after the counts, as round 4 did (A/B and the tests' second path).
  // (=2, a testing aid: also with ONE rank, which then owns every cell -- the export and the exchange run as they do with more, over RCCL on a one-GPU box)
  bool shardInput = (shardCount > 1 || (getenv("T4_SHARD_INPUT") && atoi(getenv("T4_SHARD_INPUT")) == 2 && hasBarcode && !keepMissingBarcode)) && !lateShard &&
                    (!rcclIdPath.empty() || !gatherDir.empty()) && !(getenv("T4_SHARD_INPUT") && atoi(getenv("T4_SHARD_INPUT")) == 0);
  // (the pass ahead of the loop reads the barcode file a first time: a FIFO, a process substitution or /dev/stdin would be drained by
  // it. Whether every barcode file is a regular file follows from argv alone, so every rank decides alike: round 4's way then --
  // the input phases over the whole sample on every rank, one read of every file. ADVICE r5.)
  if (shardInput)
    for (const std::string &f : barcodeFile.files) {
      struct stat sb;
      if (stat(f.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) {
        shardInput = false;
        PrintLog("The barcode file %s cannot be read twice (not a regular file): the input is not dealt out by cells, every rank reads the whole sample.", f.c_str());
        break;
      }
    }
  int ownLo = 0, ownHi = 0;   // this rank's barcode numbers [ownLo, ownHi)
  long long ownPairs = 0, allPairs = 0;
  if (shardInput) {
    ThreadedSeqReader pre;
    pre.files = barcodeFile.files;
    ThreadedSeqReader::Block b;
    StrNumbering numbers;
    std::vector<long long> per;
    while (pre.nextBlock(b))
      for (const ThreadedSeqReader::Rec &r : b) {
        if (r.seq == "missing_barcode" && !keepMissingBarcode) continue;
        bool isNew = false;
        const int x = numbers.number(r.seq, isNew);
        if (x >= (int)per.size()) per.push_back(1); else ++per[(size_t)x];
        ++allPairs;
      }
    const size_t nb = per.size();
    auto firstBarcodeOf = [&](int r) {
      if (r >= shardCount) return nb;
      const long long target = allPairs * r / shardCount;
      long long cum = 0;
      size_t x = 0;
      while (x < nb && cum < target) cum += per[x++];
      return x;
    };
    ownLo = (int)firstBarcodeOf(shardRank); ownHi = (int)firstBarcodeOf(shardRank + 1);
    for (int x = ownLo; x < ownHi; ++x) ownPairs += per[(size_t)x];
    PrintLog("Cells %d-%d of %d are this rank's (%lld of %lld read pairs by the barcode file): their pairs alone are processed and counted here.", ownLo, ownHi, (int)nb, ownPairs, allPairs);
  }
  std::vector<std::string> barcodeIntToStr;
  std::vector<int> barcodePairCount;   // main.cpp:822-828 (only counted under --contigMinCov)
  // ---- the device path of the input loop (T4_GPU_PARSE=1, the switch of the stage-0 extractor; opt-in): the two mate files go to the
  // device piece by piece as bytes. The device finds the records and validates them (t4_text_scan), and runs ProcessRead on the pairs
  // where they lie (t4_text_process_pairs) -- no host thread splits the text, and nothing is marshalled. The host numbers barcodes
  // and UMIs (small files, their readers as below), sets a skip byte for every pair that is dropped or another rank's, and builds
  // the read records of the pairs that are left straight from the piece (text_records.h). It takes text for which "four lines per
  // record" and SeqReader mean the same; at the first piece that is anything else everything gathered so far is dropped and the
  // whole input goes through the host loop below, which has not read a byte by then (so the files must be readable twice).
  const bool wantTextPath = getenv("T4_GPU_PARSE") && atoi(getenv("T4_GPU_PARSE")) == 1;
  bool textPath = false;
  // T4_TEXT_COUNTS=1 (opt-in, looked at on the device text path only): the 21-mers are counted piece by piece from the text the device
  // holds -- the pairs of a piece after ProcessRead become a batch with their qualities where they lie (t4_text_pairs_batch), no base and
  // no quality is uploaded a second time. The batches are kept for the statistics pass under the rule of the uploaded chunks below
  // (keepBatches), and when no reads are dealt to other ranks after the counts. A -c file or T4_GPU_KMERCOUNT=0 leave it off; a piece
  // whose reads the device counters do not take (a read 1 with a letter other than ACGTN, a merged read beyond 384 bases) or a device
  // allocation that fails drops the counter and the batches, and the counts are taken further down as without the switch.
  const bool wantTextCounts = getenv("T4_TEXT_COUNTS") && atoi(getenv("T4_TEXT_COUNTS")) == 1;
  struct TextCounts {
    bool on = false;
    std::string offWhy;                       // why the switch does nothing in this run
    t4_kmer_counter *kc = nullptr;
    std::vector<t4_batch *> kept;             // in input order; kept[i] holds keptRows[i] reads of sortedReads, one behind the other
    std::vector<size_t> keptRows;
    bool keep = false;
    long long batches = 0, batchesKept = 0;
    double sec = 0;
    void dropKept() { for (t4_batch *b : kept) t4_batch_destroy(b); kept.clear(); keptRows.clear(); keep = false; }
    void drop(const char *why) { dropKept(); if (kc) t4_kmer_count_destroy(kc); kc = nullptr; on = false; offWhy = why; batches = batchesKept = 0; }
  } textCounts;
  if (wantTextCounts) {
    if (!kmerCountFile.empty()) textCounts.offWhy = "a -c file";
    else if (getenv("T4_GPU_KMERCOUNT") && atoi(getenv("T4_GPU_KMERCOUNT")) == 0) textCounts.offWhy = "T4_GPU_KMERCOUNT=0";
    else {
      textCounts.on = true;
      // (reads that go to other ranks after the counts -- --cellShard without the dealt-out input -- would sit in the batches)
      const bool dealtLater = shardCount > 1 && !lateShard && (!rcclIdPath.empty() || !gatherDir.empty()) && !shardInput;
      textCounts.keep = contigMinCov <= 0 && !dealtLater;
    }
  }
  {
    auto regular = [](const std::vector<std::string> &files) { for (const std::string &f : files) { struct stat sb; if (stat(f.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return false; } return true; };
    const char *hostWhy = nullptr;
    if (!wantTextPath) hostWhy = "T4_GPU_PARSE is not 1";
    else if (!hasMate || mateReads.files.empty()) hostWhy = "single-end input";
    else if (reads.files.size() != 1 || mateReads.files.size() != 1) hostWhy = "more than one file per mate";
    else if (!regular(reads.files) || !regular(mateReads.files)) hostWhy = "a read file that is not a regular file cannot be read twice";
    else if (!regular(barcodeFile.files) || !regular(umiFile.files)) hostWhy = "a barcode or UMI file that is not a regular file cannot be read twice";
    if (!hostWhy) {
      size_t pieceBytes = (size_t)16 << 20;
#ifdef T4_TEST_KNOBS
      if (getenv("T4_TEST_TEXT_PIECE")) pieceBytes = (size_t)atol(getenv("T4_TEST_TEXT_PIECE"));   // test builds: small inputs cross piece boundaries
#endif
      gpuReady();
      struct Side {
        ByteStream in;
        t4_text *tx = nullptr;
        std::vector<char> buf;
        size_t fill = 0;          // bytes of buf in use: what the last piece left over, then fresh bytes
        bool ended = false;       // the file has no bytes beyond buf[fill)
        long long recBase = 0;    // records of the file ahead of this piece
        int64_t info[5] = {0, 0, 0, -1, 0};
        std::vector<uint32_t> recStart;
      } side[2];
      // (readers of their own for the small files: the ones of the host loop stay untouched for a give-back)
      std::unique_ptr<ThreadedSeqReader> bcIn(new ThreadedSeqReader()), umiIn(new ThreadedSeqReader());
      bcIn->files = barcodeFile.files; umiIn->files = umiFile.files;
      for (int sI = 0; sI < 2; ++sI) {
        if ((rc = t4_text_create(ctx, (int64_t)pieceBytes, &side[sI].tx))) die(ctx, "t4_text_create", rc);
        side[sI].buf.resize(pieceBytes);
        side[sI].in.start(sI == 0 ? reads.files[0] : mateReads.files[0], std::max<size_t>(1, std::min<size_t>(pieceBytes / 4, (size_t)4 << 20)));
      }
      auto closeText = [&]() { for (int sI = 0; sI < 2; ++sI) { side[sI].in.finish(); t4_text_destroy(side[sI].tx); side[sI].tx = nullptr; } bcIn.reset(); umiIn.reset(); };
      auto unevenText = [&](const char *what) { fprintf(stderr, "%s\n", what); closeText(); if (initThread.joinable()) initThread.join(); exit(1); };
      auto now = []() { return std::chrono::steady_clock::now(); };
      auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
      double secWait = 0, secScan = 0, secNumber = 0, secPairs = 0, secBuild = 0;
      int fallStatus = 0, fallSide = 0; long long fallRec = -1;
      std::vector<uint8_t> skip;
      std::vector<int> bc, umi;
      std::vector<int32_t> meta;
      std::vector<char> outR, outQ;
      const size_t PP_CHUNK = 1024;
      for (;;) {
        auto t0 = now();
        for (int sI = 0; sI < 2; ++sI) {
          Side &sd = side[sI];
          if (!sd.ended) sd.fill += sd.in.take(sd.buf.data() + sd.fill, pieceBytes - sd.fill, &sd.ended);
          if (sd.in.failed) { fprintf(stderr, "Could not open %s\n", sd.in.path.c_str()); closeText(); if (initThread.joinable()) initThread.join(); exit(EXIT_FAILURE); }
        }
        secWait += since(t0); t0 = now();
        for (int sI = 0; sI < 2 && !fallStatus; ++sI) {
          Side &sd = side[sI];
          if ((rc = t4_text_scan(sd.tx, sd.buf.data(), (int64_t)sd.fill, sd.ended ? 1 : 0, sd.info))) die(ctx, "t4_text_scan", rc);
          if (sd.info[2]) { fallStatus = (int)sd.info[2]; fallRec = sd.recBase + sd.info[3]; fallSide = sI; }
        }
        secScan += since(t0);
        if (fallStatus) break;
        const int64_t n1 = side[0].info[0], n2 = side[1].info[0], m = std::min(n1, n2);
        if (m == 0) {
          if (n1 == 0 && side[0].ended) break;   // every read has been seen (what the mate file has beyond them is not looked at, as on the host path)
          if (n2 == 0 && side[1].ended) unevenText("The mate-pair read file has fewer reads than the first read file.");
          fallStatus = 9; fallSide = n1 == 0 ? 0 : 1; fallRec = side[fallSide].recBase;   // a record that does not fit a piece
          break;
        }
        t0 = now();
        const size_t n = (size_t)m;
        for (int sI = 0; sI < 2; ++sI) {
          side[sI].recStart.resize(n + 1);
          if ((rc = t4_text_records(side[sI].tx, 0, m, side[sI].recStart.data(), nullptr))) die(ctx, "t4_text_records", rc);
        }
        secScan += since(t0); t0 = now();
        // barcodes and UMIs of the m pairs, numbered in order of first appearance; the skip bytes (main.cpp:799-842, as the host loop)
        bc.assign(n, -1); umi.assign(n, -1); skip.assign(n, 0);
        if (hasBarcode)
          for (size_t i = 0; i < n; ++i) {
            if (!bcIn->next()) unevenText("The barcode file has fewer records than the read file.");
            const std::string &bs = bcIn->seq;
            if (bs == "missing_barcode" && !keepMissingBarcode) { skip[i] = 1; continue; }
            bool isNew = false;
            const int barcode = barcodeNumbers.number(bs, isNew);
            if (isNew) barcodeIntToStr.push_back(bs);
            if (contigMinCov > 0) { if (barcode >= (int)barcodePairCount.size()) barcodePairCount.push_back(1); else ++barcodePairCount[barcode]; }
            bc[i] = barcode;
            if (shardInput && (barcode < ownLo || barcode >= ownHi)) skip[i] = 2;
          }
        if (hasUmi)
          for (size_t i = 0; i < n; ++i) {
            if (!umiIn->next()) unevenText("The UMI file has fewer records than the read file.");
            if (skip[i] == 1) continue;
            bool isNew = false;
            umi[i] = umiNumbers.number(umiIn->seq, isNew);
          }
        size_t kept = 0;
        for (size_t i = 0; i < n; ++i) if (skip[i] != 1) {
          if (firstReadLen == -1) {
            TextRecord tr;
            firstReadLen = cutTextRecord(side[0].buf.data(), side[0].fill, side[0].recStart.data(), i, tr) ? (int)tr.seqLen : 0;
            if (firstReadLen > 200) { fprintf(stderr, "trust4-hip: long-read mode (first read > 200 bp, main.cpp:1467-1481) is not built.\n"); closeText(); if (initThread.joinable()) initThread.join(); return EXIT_FAILURE; }
          }
          ++kept;
        }
        const int before = nIn;
        nIn += (int)(kept * 2);
        for (int t = before / 100000 + 1; t <= nIn / 100000; ++t) PrintLog("Read in and count kmers for %d reads.", t * 100000);
        secNumber += since(t0); t0 = now();
        // ProcessRead of the pairs on the device, where they lie
        meta.resize(n * 4);
        const size_t room = (side[0].fill + side[1].fill) / 2;
        if (outR.size() < room) { outR.resize(room); outQ.resize(room); }
        int64_t outBytes = 0;
        if ((rc = t4_text_process_pairs(side[0].tx, side[1].tx, 0, 0, m, skip.data(), meta.data(), outR.data(), outQ.data(), (int64_t)room, &outBytes))) die(ctx, "t4_text_process_pairs", rc);
        for (size_t i = 0; i < n; ++i) if (!skip[i]) ++ppKinds[meta[i * 4] & 3];
        secPairs += since(t0); t0 = now();
        // the read records of the pairs that are left, on the host threads, in input order
        const size_t nChunks = (n + PP_CHUNK - 1) / PP_CHUNK;
        std::vector<std::vector<SortRead>> &outs = chunkOuts;
        if (outs.size() < nChunks) outs.resize(nChunks);
        std::atomic<bool> badCut(false);
        double secCountPiece = 0;   // T4_TEXT_COUNTS=1: the seconds of this piece's count, which are not the record building's
        parallelFor((long long)nChunks, threadCnt, [&](long long c) {
          std::vector<SortRead> &out = outs[(size_t)c];
          const size_t lo = (size_t)c * PP_CHUNK, hi = lo + PP_CHUNK < n ? lo + PP_CHUNK : n;
          out.clear();
          out.reserve((hi - lo) * 2 + 2);
          TextRecord a, b;
          for (size_t i = lo; i < hi; ++i) {
            if (skip[i]) continue;
            const int len = meta[i * 4 + 1], fl = meta[i * 4 + 2], at = meta[i * 4 + 3];
            if (!cutTextRecord(side[0].buf.data(), side[0].fill, side[0].recStart.data(), i, a) ||
                !cutTextRecord(side[1].buf.data(), side[1].fill, side[1].recStart.data(), i, b)) { badCut.store(true); continue; }
            if (fl & 1) {
              out.emplace_back();
              SortRead &r1 = out.back();
              textRecordId(a, reads.stripMateSuffix, r1.id);
              if (fl & 16) { r1.read.assign(outR.data() + at, (size_t)len); if (fl & 8) r1.qual.assign(outQ.data() + at, (size_t)len); }
              else { r1.read.assign(a.seq, a.seqLen); r1.qual.assign(a.qual, a.qualLen); }
              r1.hasQual = (fl & 8) != 0;
              r1.barcode = bc[i]; r1.umi = umi[i];
              if (fl & 4) { SortRead w = r1; w.id += ".1"; out.push_back(std::move(w)); }
            }
            if (fl & 2) {
              out.emplace_back();
              SortRead &r2 = out.back();
              textRecordId(b, mateReads.stripMateSuffix, r2.id);
              r2.read.assign(b.seq, b.seqLen); r2.qual.assign(b.qual, b.qualLen);
              for (char &ch : r2.read) if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' && ch != 'N') ch = 'N';   // what two reverse complements leave
              r2.hasQual = true;
              r2.barcode = bc[i]; r2.umi = umi[i];
            }
          }
        });
        if (badCut.load()) { fprintf(stderr, "trust4-hip: T4_GPU_PARSE: the record table of a piece does not fit its text\n"); closeText(); return EXIT_FAILURE; }
        {
          std::vector<size_t> first(nChunks + 1, sortedReads.size());
          for (size_t c = 0; c < nChunks; ++c) first[c + 1] = first[c] + outs[c].size();
          sortedReads.resize(first[nChunks]);
          parallelFor((long long)nChunks, threadCnt, [&](long long c) {
            std::vector<SortRead> &v = outs[(size_t)c];
            for (size_t j = 0; j < v.size(); ++j) sortedReads[first[(size_t)c] + j] = std::move(v[j]);
            v.clear();
          });
          if (textCounts.on) {   // T4_TEXT_COUNTS=1: the reads just appended, counted where the device holds them
            const auto tc0 = now();
            const size_t appended = first[nChunks] - first[0];
            int64_t binfo[4] = {0, 0, 0, 0};
            t4_batch *tb = nullptr;
            const char *why = nullptr;
            std::string whyText;
            auto soft = [&](const char *call, const char *unsupported) {   // what sends the run back to the uploaded reads; anything else is an error of the run
              // (T4_ERR_HIP is every HIP error: only memory that could not be had leaves the device fit for the path without the switch)
              const char *msg = rc == T4_ERR_HIP ? t4_last_error(ctx) : "";
              const bool noMemory = strstr(msg, "hipMalloc") || strstr(msg, "hipHostMalloc") || strstr(msg, "no device memory");
              if (rc == T4_ERR_HIP && noMemory) { whyText = std::string("a device allocation failed: ") + msg; why = whyText.c_str(); }
              else if (rc == T4_ERR_UNSUPPORTED) why = unsupported;
              else if (rc) die(ctx, call, rc);
            };
            rc = t4_text_pairs_batch(side[0].tx, side[1].tx, 0, 0, m, trimLevel != 0 ? 1 : 0, &tb, binfo);
            soft("t4_text_pairs_batch", "a merged read beyond 384 bases");
            if (!why && binfo[3]) why = "a letter other than ACGTN in a read 1";
            if (!why && (size_t)binfo[0] != appended) {
              fprintf(stderr, "trust4-hip: T4_TEXT_COUNTS: the device made %lld reads of a piece, the host %zu\n", (long long)binfo[0], appended);
              closeText(); if (initThread.joinable()) initThread.join(); return EXIT_FAILURE;
            }
            if (!why && !textCounts.kc) { rc = t4_kmer_count_create(ctx, 21, 1ll << 21, 0, &textCounts.kc); soft("t4_kmer_count_create", "the count table"); }
            // (the size of the read set is not known while the pieces stream: room for this piece's k-mers, fewer than its bases)
            if (!why) { rc = t4_kmer_count_reserve(textCounts.kc, binfo[1]); soft("t4_kmer_count_reserve", "the count table is full"); }
            if (!why) { rc = t4_kmer_count_add(textCounts.kc, tb); soft("t4_kmer_count_add", "the count table is full"); }
            if (why) {
              if (tb) t4_batch_destroy(tb);
              textCounts.drop(why);
            } else {
              ++textCounts.batches;
              if (textCounts.keep && sortedReads.size() > ((size_t)16 << 20)) textCounts.dropKept();   // (60 B per read on the device, and their qualities)
              if (textCounts.keep) { textCounts.kept.push_back(tb); textCounts.keptRows.push_back(appended); }
              else t4_batch_destroy(tb);
            }
            secCountPiece = since(tc0);
            textCounts.sec += secCountPiece;
          }
        }
        for (int sI = 0; sI < 2; ++sI) {   // what the piece holds beyond record m goes to the front of the next one
          Side &sd = side[sI];
          const size_t used = sd.recStart[n];
          memmove(sd.buf.data(), sd.buf.data() + used, sd.fill - used);
          sd.fill -= used; sd.recBase += m;
        }
        secBuild += since(t0) - secCountPiece;
      }
      const std::string fallFile = side[fallSide].in.path;
      closeText();
      if (!fallStatus) {
        textPath = true;
        if (getenv("T4_TIMING")) {
          PrintLog("path: device text (T4_GPU_PARSE=1, pieces of %zu bytes)", pieceBytes);
          PrintLog("timing: device text: %.2f s waiting for pieces, %.2f s finding the records, %.2f s numbering, %.2f s ProcessRead on the device, %.2f s building the read records", secWait, secScan, secNumber, secPairs, secBuild);
        }
        secProcess = secPairs; secMerge = secBuild;
        if (textCounts.on && !textCounts.kc) textCounts.drop("the input holds no pair");
        textCounts.batchesKept = (long long)textCounts.kept.size();
        if (textCounts.on && getenv("T4_TIMING"))
          PrintLog("timing: 21-mers counted from the device's reads (T4_TEXT_COUNTS=1): %lld batches in %.2f s of the input loop, %lld kept for the statistics", textCounts.batches, textCounts.sec, textCounts.batchesKept);
      } else {
        if (textCounts.on) textCounts.drop("the input went through the host loop");   // (the counter and the batches go with everything else)
        PrintLog("T4_GPU_PARSE: status %d at record %lld of %s; the whole input goes through the host loop", fallStatus, fallRec, fallFile.c_str());
        hostWhy = "the device path gave the input back";
        // (everything the loop has gathered goes: the host loop starts from nothing, as without the switch)
        std::vector<SortRead>().swap(sortedReads);
        barcodeNumbers = StrNumbering(); umiNumbers = StrNumbering();
        barcodeIntToStr.clear(); barcodePairCount.clear();
        firstReadLen = -1; nIn = 0;
        for (long long &k : ppKinds) k = 0;
      }
    }
    if (hostWhy && getenv("T4_TIMING")) PrintLog("path: host (%s)", hostWhy);
    if (hostWhy && textCounts.on) textCounts.drop("the input went through the host loop");
  }
  if (wantTextCounts && !textCounts.on) PrintLog("T4_TEXT_COUNTS: the 21-mers are counted from the reads of the host's list as without the switch (%s)", textCounts.offWhy.c_str());
  if (!textPath) {
    ThreadedSeqReader::Block bR, bM, bB, bU;
    auto uneven = [&](const char *what) { fprintf(stderr, "%s\n", what); if (processThread.joinable()) processThread.join(); if (initThread.joinable()) initThread.join(); exit(1); };
    while (reads.nextBlock(bR)) {
      Unit u;
      u.r.swap(bR);
      const size_t n = u.r.size();
      if (hasMate) {
        // (records of the mate file beyond the last read of the first file are ignored, as the reference's `while ( reads.Next() )`
        // ignores them, main.cpp:787-800; a mate file that ends early is refused -- the reference reads stale buffers there)
        if (!mateReads.nextBlock(bM) || bM.size() < n) uneven("The mate-pair read file has fewer reads than the first read file.");
        if (bM.size() > n) bM.resize(n);
        u.m.swap(bM);
      }
      u.bc.assign(n, -1); u.umi.assign(n, -1); u.skip.assign(n, 0);
      if (hasBarcode) {   // main.cpp:799-828
        if (!barcodeFile.nextBlock(bB) || bB.size() < n) uneven("The barcode file has fewer records than the read file.");
        for (size_t i = 0; i < n; ++i) {
          const std::string &bs = bB[i].seq;
          if (bs == "missing_barcode" && !keepMissingBarcode) { u.skip[i] = 1; continue; }
          int barcode;
          bool isNew = false;
          barcode = barcodeNumbers.number(bs, isNew);
          if (isNew) barcodeIntToStr.push_back(bs);
          if (contigMinCov > 0) { if (barcode >= (int)barcodePairCount.size()) barcodePairCount.push_back(1); else ++barcodePairCount[barcode]; }
          u.bc[i] = barcode;
          if (shardInput && (barcode < ownLo || barcode >= ownHi)) u.skip[i] = 2;   // another rank's cell: the record is numbered (barcode, UMI) and let go
        }
      }
      if (hasUmi) {       // main.cpp:831-842
        if (!umiFile.nextBlock(bU) || bU.size() < n) uneven("The UMI file has fewer records than the read file.");
        for (size_t i = 0; i < n; ++i) {
          if (u.skip[i] == 1) continue;
          bool isNew = false;
          u.umi[i] = umiNumbers.number(bU[i].seq, isNew);
        }
      }
      size_t kept = 0, keptHere = 0;
      for (size_t i = 0; i < n; ++i) if (u.skip[i] != 1) {
        if (!u.skip[i]) ++keptHere;
        if (firstReadLen == -1) {
          firstReadLen = (int)u.r[i].seq.size();
          if (firstReadLen > 200) { fprintf(stderr, "trust4-hip: long-read mode (first read > 200 bp, main.cpp:1467-1481) is not built.\n"); if (processThread.joinable()) processThread.join(); if (initThread.joinable()) initThread.join(); return EXIT_FAILURE; }
        }
        ++kept;
      }
      const int before = nIn;
      nIn += (int)(kept * (hasMate ? 2 : 1));
      for (int t = before / 100000 + 1; t <= nIn / 100000; ++t) PrintLog("Read in and count kmers for %d reads.", t * 100000);
      if (!reservedReadList && n > 0) {   // room for the whole input, told from the first block's bytes per record and the size of the file
        reservedReadList = true;
        size_t bytes = 0;
        for (size_t i = 0; i < n; ++i) bytes += u.r[i].id.size() + u.r[i].seq.size() + (u.r[i].hasQual ? u.r[i].qual.size() + 3 : 0) + 3;
        bool plain = true;
        double fileBytes = 0;
        for (const std::string &f : reads.files) {
          struct stat st;
          if (f.size() > 3 && f.compare(f.size() - 3, 3, ".gz") == 0) plain = false;
          else if (stat(f.c_str(), &st) == 0 && S_ISREG(st.st_mode)) fileBytes += (double)st.st_size;
          else plain = false;
        }
        if (plain && bytes > 0) {
          const double recs = fileBytes / ((double)bytes / (double)n) * 1.03 + 1024;
          const double want = recs * (hasMate ? 2.0 : 1.0) * (shardInput && allPairs > 0 ? (double)ownPairs / (double)allPairs * 1.05 : 1.0);
          if (want < 2.0e9) sortedReads.reserve((size_t)want);
        }
      }
      unitPairs += keptHere;
      units.push_back(std::move(u));
      if (unitPairs >= BLOCK || (shardInput && units.size() >= 24)) flushBlock();   // (blocks of other ranks' cells go back to their readers before long)
    }
  }
  flushBlock();
  { const auto tw = std::chrono::steady_clock::now(); if (processThread.joinable()) processThread.join(); secWaitProcess += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count(); }
  if (getenv("T4_TIMING")) PrintLog("timing: input loop %.2f s, of which %.2f s waiting for the ProcessRead of the batch before", std::chrono::duration<double>(std::chrono::steady_clock::now() - tInput0).count(), secWaitProcess);
  if (gpuProcess || textPath) PrintLog("ProcessRead on the device: %lld pairs stay as they are, %lld read-through, %lld merged, %lld with one mate for both", ppKinds[0], ppKinds[1], ppKinds[2], ppKinds[3]);
  if (gpuProcess && ppBlocksOnHost) PrintLog("ProcessRead: %lld blocks held a mate beyond the device path's length and were processed on the host threads", ppBlocksOnHost);
  if (getenv("T4_TIMING")) PrintLog("timing: input parsed and mates processed (ProcessRead %.2f s on %d threads, merge %.2f s)", secProcess, threadCnt, secMerge);
  const auto tInputEnd = std::chrono::steady_clock::now();
  int readCnt = (int)sortedReads.size();
  int maxReadLen = 0;
  for (const SortRead &r : sortedReads) if ((int)r.read.size() > maxReadLen) maxReadLen = (int)r.read.size();
  kmerCount.maxReadLen = maxReadLen;   // KmerCount::SetBuffer (main.cpp:979)
  if (!kmerCountFile.empty()) {   // -c: counts come from a k-mer counter's dump instead (main.cpp:694-699)
    if (!kmerCount.addCountFromFile(kmerCountFile.c_str())) { fprintf(stderr, "Could not open %s\n", kmerCountFile.c_str()); if (initThread.joinable()) initThread.join(); return EXIT_FAILURE; }
    PrintLog("Read in the kmer count information from %s", kmerCountFile.c_str());
  }
  // The 21-mer counts and the count statistics on the device (t4_kmer_count_*). The device path takes: reads of at most 384 bp over
  // ACGTN, qualities on every read or on none (a -c file is loaded into the device table as it is).
  t4_kmer_counter *gpuKc = nullptr;
  bool gpuQual = false;
  const size_t KC_CHUNK = 1u << 22;
  std::string scratchBases; std::vector<int64_t> scratchOff;   // the reads of a chunk side by side: one buffer for every upload of the run (its pages are touched once)
  std::vector<t4_batch *> countedBatches;   // the chunks as the count pass uploaded them, kept for the statistics pass when nothing changes in between
  auto uploadChunk = [&](size_t lo, size_t hi, std::string &bases, std::vector<int64_t> &off, bool withBarcodes = false) -> t4_batch * {
    const size_t n = hi - lo;
    off.resize(n + 1);
    off[0] = 0;
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)sortedReads[lo + i].read.size();
    bases.resize((size_t)off[n]);
    std::vector<int32_t> bcs(withBarcodes ? n : 0);
    parallelFor((long long)n, threadCnt, [&](long long i) {   // the reads side by side (the copy of 150 bytes per read is all there is to do)
      const std::string &r = sortedReads[lo + (size_t)i].read;
      if (!r.empty()) memcpy(&bases[(size_t)off[(size_t)i]], r.data(), r.size());
      if (withBarcodes) bcs[(size_t)i] = sortedReads[lo + (size_t)i].barcode;
    });
    t4_batch *b = nullptr;
    if ((rc = t4_reads_upload(ctx, bases.data(), off.data(), withBarcodes ? bcs.data() : nullptr, (int64_t)(hi - lo), &b))) die(ctx, "t4_reads_upload", rc);
    return b;
  };
  bool gpuKmerCounts = false;   // the device path was taken: the barcode-wise counts follow it
  // Default since round 3 (1 M barcoded pairs: 23.9 -> 21.2 s, profiles/r03l_*): on the device whenever the input is what the device
  // path takes; T4_GPU_KMERCOUNT=0 keeps the host threads, =1 insists (and says why it cannot).
  bool wantGpuKc = false, insistGpuKc = false;
  if (textCounts.on) {   // counted piece by piece in the input loop: every read has qualities (FASTQ text), none is beyond 384 bases or holds another letter
    gpuKc = textCounts.kc; textCounts.kc = nullptr;
    gpuKmerCounts = true; gpuQual = trimLevel != 0;
    if (!textCounts.keep) textCounts.dropKept();
    if (readCnt <= 0) { t4_kmer_count_destroy(gpuKc); gpuKc = nullptr; gpuKmerCounts = false; gpuQual = false; textCounts.dropKept(); }   // (nothing was counted)
  } else if (readCnt > 0) {
    const char *ev = getenv("T4_GPU_KMERCOUNT");
    if (ev) { wantGpuKc = atoi(ev) != 0; insistGpuKc = wantGpuKc; }
    else {
      std::atomic<long long> nQualA(0);
      std::atomic<bool> other(false);
      if (maxReadLen <= 384)
        parallelFor((long long)sortedReads.size(), threadCnt, [&](long long i) {
          const SortRead &r = sortedReads[(size_t)i];
          if (r.hasQual) nQualA.fetch_add(1, std::memory_order_relaxed);
          for (char ch : r.read) if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' && ch != 'N') { other.store(true, std::memory_order_relaxed); break; }
        });
      const size_t nQual = (size_t)nQualA.load();
      wantGpuKc = maxReadLen <= 384 && !other.load() && (trimLevel == 0 || nQual == 0 || nQual == sortedReads.size());
    }
  }
  if (wantGpuKc) {
    size_t nQual = 0;
    long long kmers = 0;
    for (const SortRead &r : sortedReads) { if (r.hasQual) ++nQual; if ((int)r.read.size() >= 21) kmers += (long long)r.read.size() - 20; }
    if (maxReadLen > 384) { fprintf(stderr, "trust4-hip: T4_GPU_KMERCOUNT takes reads of at most 384 bp (longest here: %d)\n", maxReadLen); if (initThread.joinable()) initThread.join(); return EXIT_FAILURE; }
    if (trimLevel != 0 && nQual != 0 && nQual != sortedReads.size()) { fprintf(stderr, "trust4-hip: T4_GPU_KMERCOUNT needs qualities on every read or on none\n"); if (initThread.joinable()) initThread.join(); return EXIT_FAILURE; }
    gpuQual = trimLevel != 0 && nQual == sortedReads.size();
    gpuKmerCounts = true;
    gpuReady();
    if (!kmerCountFile.empty()) { kmers = 16; for (const auto &m : kmerCount.shards) kmers += (long long)m.size(); }
    // The table is sized for every k-mer position (an upper bound of the distinct k-mers), at most 2^30 of them. When the device path
    // was chosen by default (not by T4_GPU_KMERCOUNT=1) and the table cannot be had or fills up -- a shared or smaller GPU, more than
    // 2^30 distinct 21-mers -- the counts are taken on the host threads as before round 3, with a note; =1 insists and stops.
    const char *why = nullptr;
    rc = t4_kmer_count_create(ctx, 21, kmers + 16 < (1ll << 30) ? kmers + 16 : (1ll << 30), 0, &gpuKc);
    if (rc) why = "t4_kmer_count_create";
    std::string &bases = scratchBases; std::vector<int64_t> &off = scratchOff;
    const bool keepBatches = contigMinCov <= 0 && sortedReads.size() <= ((size_t)16 << 20);   // (60 B per read on the device)
    if (!why && !kmerCountFile.empty()) {   // -c: the counts parsed from the file above, as they are (t4_kmer_count_set)
      std::vector<uint64_t> codes; std::vector<int32_t> vals;
      for (const auto &m : kmerCount.shards) for (const auto &kv : m) { codes.push_back(kv.first); vals.push_back(kv.second); }
      if ((rc = t4_kmer_count_set(gpuKc, codes.data(), vals.data(), (int64_t)codes.size()))) why = "t4_kmer_count_set";
    } else if (!why)
    for (size_t lo = 0; lo < sortedReads.size() && !why; lo += KC_CHUNK) {
      const size_t hi = lo + KC_CHUNK < sortedReads.size() ? lo + KC_CHUNK : sortedReads.size();
      t4_batch *b = uploadChunk(lo, hi, bases, off);
      if ((rc = t4_kmer_count_add(gpuKc, b))) why = "t4_kmer_count_add";
      if (keepBatches && !why) countedBatches.push_back(b); else t4_batch_destroy(b);
    }
    if (why) {
      for (t4_batch *kb : countedBatches) t4_batch_destroy(kb);
      countedBatches.clear();
      if (insistGpuKc) die(ctx, why, rc);
      fprintf(stderr, "trust4-hip: 21-mer counts on the host threads (%s: %s)\n", why, t4_last_error(ctx));
      if (gpuKc) { t4_kmer_count_destroy(gpuKc); gpuKc = nullptr; }
      gpuKmerCounts = false; gpuQual = false;
      if (kmerCountFile.empty()) kmerCount.addCountAll((long long)sortedReads.size(), threadCnt, [&](long long i) -> const std::string & { return sortedReads[(size_t)i].read; });
    }
  } else if (kmerCountFile.empty() && !textCounts.on)
  kmerCount.addCountAll((long long)sortedReads.size(), threadCnt, [&](long long i) -> const std::string & { return sortedReads[(size_t)i].read; });
  if (getenv("T4_TIMING")) PrintLog("timing: 21-mers counted%s (%.2f s since the input ended)", gpuKc ? " (on the device)" : "", std::chrono::duration<double>(std::chrono::steady_clock::now() - tInputEnd).count());
  gpuReady();
  if (shardInput && kmerCountFile.empty()) {
    // The counts of the whole sample: every rank's pairs to every rank (payload: n, n codes, n counts), the others' added where this
    // rank's table holds the k-mer -- its reads' k-mers are all there, and nothing else is ever looked up.
    const auto tm0 = std::chrono::steady_clock::now();
    std::string mine;
    int64_t n = 0;
    if (gpuKc) {
      if ((rc = t4_kmer_count_export(gpuKc, nullptr, nullptr, 0, &n))) die(ctx, "t4_kmer_count_export", rc);
      mine.resize(8 + (size_t)n * 12);
      if (n > 0 && (rc = t4_kmer_count_export(gpuKc, (uint64_t *)(&mine[8]), (int32_t *)(&mine[8 + (size_t)n * 8]), n, &n))) die(ctx, "t4_kmer_count_export", rc);
    } else {
      for (const auto &m : kmerCount.shards) n += (int64_t)m.size();
      mine.resize(8 + (size_t)n * 12);
      uint64_t *codes = (uint64_t *)(&mine[8]); int32_t *vals = (int32_t *)(&mine[8 + (size_t)n * 8]);
      size_t at = 0;
      for (const auto &m : kmerCount.shards) for (const auto &kv : m) { codes[at] = kv.first; vals[at] = kv.second; ++at; }
    }
    memcpy(&mine[0], &n, 8);
    std::vector<std::string> got;
    if (!exchange(mine, true, got)) { fprintf(stderr, "trust4-hip: the exchange of the 21-mer counts failed\n"); return EXIT_FAILURE; }
    std::string().swap(mine);
    long long taken = 0;
    for (int r = 0; r < shardCount; ++r) {
      if (r == shardRank || testNoCountMerge) continue;   // (testing aid: the negative control of tests/test_dist_gloo.py -- without the other ranks' counts the read statistics are wrong)
      std::string &g = got[(size_t)r];
      int64_t m = 0;
      if (g.size() >= 8) memcpy(&m, g.data(), 8);
      if (g.size() < 8 || m < 0 || g.size() != 8 + (size_t)m * 12) { fprintf(stderr, "trust4-hip: rank %d sent %zu bytes of 21-mer counts that do not hold %lld pairs\n", r, g.size(), (long long)m); return EXIT_FAILURE; }
      const uint64_t *codes = (const uint64_t *)(g.data() + 8); const int32_t *vals = (const int32_t *)(g.data() + 8 + (size_t)m * 8);
      if (gpuKc) { if ((rc = t4_kmer_count_merge(gpuKc, codes, vals, m, 1))) die(ctx, "t4_kmer_count_merge", rc); }
      else
        parallelFor((long long)kmerCount.shards.size(), threadCnt, [&](long long sh) {
          auto &tab = kmerCount.shards[(size_t)sh];
          const bool one = kmerCount.shards.size() == 1;
          for (int64_t i = 0; i < m; ++i) {
            if (!one && (long long)kmerCount.shardOf(codes[i]) != sh) continue;
            auto it = tab.find(codes[i]);
            if (it != tab.end()) it->second += vals[i];
          }
        });
      taken += (long long)m;
      std::string().swap(g);
    }
    PrintLog("21-mer counts of the whole sample: %lld pairs of this rank's table went to the other ranks, %lld of theirs were looked at.", (long long)n, taken);
    if (getenv("T4_TIMING")) PrintLog("timing: counts of the ranks put together in %.2f s", std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count());
  }
  auto writeEmpty = [&](const char *suffix) { FILE *fp = fopen((outputPrefix + suffix).c_str(), "w"); if (fp) fclose(fp); };
  // (a rank of a run whose input is dealt out by cells may hold no read at all: it goes on, as a rank without cells always has, and takes part in the exchanges)
  if (readCnt <= 0 && !(shardInput && allPairs > 0)) { writeEmpty("_raw.out"); writeEmpty("_assembled_reads.fa"); writeEmpty("_final.out"); return 0; }

  if (contigMinCov > 0) {   // reads of barcodes with too few read pairs are dropped, after their k-mers were counted (main.cpp:951-977)
    std::vector<SortRead> kept;
    for (SortRead &r : sortedReads) if (!(r.barcode != -1 && barcodePairCount[r.barcode] < contigMinCov)) kept.push_back(std::move(r));
    sortedReads.swap(kept);
    readCnt = (int)sortedReads.size();
  }
  // ---- --cellShard R/N, early (round 4). The 21-mer counts above need every read of the sample; nothing after them does: statistics,
  // trimming, sorting, rough annotation, barcode-wise counts and the cell pass of a cell look at that cell's reads only. So the cells are
  // dealt to the ranks HERE -- contiguous ranges of the barcode numbers (= the order of the output) with about the same number of reads --
  // and every rank lets go of the other ranks' reads. What stays replicated: parsing, ProcessRead, the global counts. One coupling
  // between neighbouring cells exists (good-candidate propagation over identical boundary reads, see the walks below); it is looked
  // for across the rank boundaries once the reads are in their final order, and a run that has it starts over with --lateShard.
  if (shardCount > 1) mark("counted_all_reads");   // (what comes before is replicated on every rank of a sharded run)
  const bool earlyShard = shardCount > 1 && !lateShard && (!rcclIdPath.empty() || !gatherDir.empty());   // (the boundary check needs the transport; shard files without one: as before)
  if (earlyShard && shardInput) PrintLog("Cells %d-%d of %d are this rank's (%d reads).", ownLo, ownHi, (int)barcodeIntToStr.size(), readCnt);   // (the input loop kept nothing else)
  else if (earlyShard) {
    const size_t nb = barcodeIntToStr.size();
    std::vector<long long> per(nb, 0);
    for (const SortRead &r : sortedReads) if (r.barcode >= 0) ++per[(size_t)r.barcode];
    const long long total = (long long)sortedReads.size();
    auto firstBarcodeOf = [&](int r) {   // barcodes [firstBarcodeOf(r), firstBarcodeOf(r + 1)) are rank r's
      if (r >= shardCount) return nb;
      const long long target = total * r / shardCount;
      long long cum = 0;
      size_t b = 0;
      while (b < nb && cum < target) cum += per[b++];
      return b;
    };
    const int bLo = (int)firstBarcodeOf(shardRank), bHi = (int)firstBarcodeOf(shardRank + 1);
    std::vector<SortRead> kept;
    size_t mine = 0;
    for (const SortRead &r : sortedReads) if (r.barcode >= bLo && r.barcode < bHi) ++mine;
    kept.reserve(mine);
    for (SortRead &r : sortedReads) if (r.barcode >= bLo && r.barcode < bHi) kept.push_back(std::move(r));
    sortedReads.swap(kept);
    readCnt = (int)sortedReads.size();
    for (t4_batch *kb : countedBatches) t4_batch_destroy(kb);   // (the chunks of the count pass held every rank's reads)
    countedBatches.clear();
    textCounts.dropKept();
    PrintLog("Cells %d-%d of %d are this rank's (%d of %lld reads).", bLo, bHi, (int)nb, readCnt, total);
  }
  // ---- count statistics + quality trimming (main.cpp:980-1061)
  if (gpuKc) {
    std::string &bases = scratchBases; std::string quals; std::vector<int64_t> &off = scratchOff;
    std::vector<int32_t> mn, md, nl; std::vector<float> av;
    auto takeStats = [&](size_t lo, size_t n) {
      parallelFor((long long)n, threadCnt, [&](long long ii) {
        const size_t i = (size_t)ii;
        SortRead &r = sortedReads[lo + i];
        r.minCnt = mn[i]; r.medianCnt = md[i]; r.avgCnt = av[i];
        if ((size_t)nl[i] < r.read.size()) r.read.resize((size_t)nl[i]);
        r.qual.clear(); r.qual.shrink_to_fit(); r.hasQual = false;
        if (r.read.empty()) r.dead = true;
      });
    };
    // T4_TEXT_COUNTS=1 with its batches kept: they hold the reads of the list in its order, with their qualities -- nothing is uploaded
    const bool resident = !textCounts.kept.empty();
    if (resident) {
      size_t lo = 0;
      for (size_t bi = 0; bi < textCounts.kept.size(); ++bi) {
        const size_t n = textCounts.keptRows[bi];
        if (lo + n > sortedReads.size()) break;
        mn.resize(n); md.resize(n); nl.resize(n); av.resize(n);
        if ((rc = t4_kmer_count_stats_resident(gpuKc, textCounts.kept[bi], gpuQual ? 1 : 0, mn.data(), md.data(), av.data(), nl.data()))) die(ctx, "t4_kmer_count_stats_resident", rc);
        t4_batch_destroy(textCounts.kept[bi]); textCounts.kept[bi] = nullptr;
        takeStats(lo, n);
        lo += n;
      }
      if (lo != sortedReads.size() || textCounts.kept.back()) {
        fprintf(stderr, "trust4-hip: T4_TEXT_COUNTS: the kept batches hold %zu reads or more, the list %zu\n", lo, sortedReads.size());
        if (initThread.joinable()) initThread.join();
        return EXIT_FAILURE;
      }
      textCounts.kept.clear(); textCounts.keptRows.clear();
    }
    const bool reuse = !countedBatches.empty();
    for (size_t lo = 0, ci = 0; !resident && lo < sortedReads.size(); lo += KC_CHUNK, ++ci) {
      const size_t hi = lo + KC_CHUNK < sortedReads.size() ? lo + KC_CHUNK : sortedReads.size(), n = hi - lo;
      t4_batch *b = reuse ? countedBatches[ci] : uploadChunk(lo, hi, bases, off);
      if (gpuQual && reuse) {   // (the offsets of the qualities: where the bases of the chunk stood)
        off.resize(n + 1); off[0] = 0;
        for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)sortedReads[lo + i].read.size();
      }
      if (gpuQual) {   // (the qualities of a read stand where its bases stand: same offsets)
        quals.resize((size_t)off[n]);
        parallelFor((long long)n, threadCnt, [&](long long i) { const SortRead &r = sortedReads[lo + (size_t)i]; const size_t m = r.qual.size() < r.read.size() ? r.qual.size() : r.read.size(); if (m) memcpy(&quals[(size_t)off[(size_t)i]], r.qual.data(), m); });
      }
      mn.resize(n); md.resize(n); nl.resize(n); av.resize(n);
      if ((rc = t4_kmer_count_stats(gpuKc, b, gpuQual ? quals.data() : nullptr, gpuQual ? off.data() : nullptr, mn.data(), md.data(), av.data(), nl.data()))) die(ctx, "t4_kmer_count_stats", rc);
      t4_batch_destroy(b);
      takeStats(lo, n);
    }
    countedBatches.clear();   // (every kept batch was destroyed with its chunk above)
    t4_kmer_count_destroy(gpuKc);
    gpuKc = nullptr;
  } else
  parallelFor((long long)sortedReads.size(), threadCnt, [&](long long i) {
    SortRead &r = sortedReads[(size_t)i];
    kmerCount.statsAndTrim(r.read, (trimLevel == 0 || !r.hasQual) ? nullptr : &r.qual, r.minCnt, r.medianCnt, r.avgCnt);
    r.qual.clear(); r.qual.shrink_to_fit(); r.hasQual = false;
    if (r.read.empty()) r.dead = true;
  });
  {
    std::atomic<bool> anyDead(false);
    parallelFor((long long)sortedReads.size(), threadCnt, [&](long long i) { SortRead &r = sortedReads[(size_t)i]; if (r.dead) anyDead.store(true, std::memory_order_relaxed); else r.len = (int)r.read.size(); });
    if (anyDead.load()) {
      std::vector<SortRead> kept;
      for (SortRead &r : sortedReads) if (!r.dead) kept.push_back(std::move(r));
      sortedReads.swap(kept);
    }
    readCnt = (int)sortedReads.size();
  }
  if (getenv("T4_TIMING")) PrintLog("timing: count statistics and trimming done (%.2f s since the input ended)", std::chrono::duration<double>(std::chrono::steady_clock::now() - tInputEnd).count());
  mark("input_processed_counted");
  PrintLog("Found %i reads.", readCnt);
  kmerCount.shards.clear();
  for (int i = 0; i < readCnt; ++i) { sortedReads[i].info = i; sortedReads[i].mateIdx = -1; }
  for (int i = 0; i < readCnt - 1; ++i)
    if (sortedReads[i].id == sortedReads[i + 1].id) { sortedReads[i].mateIdx = i + 1; sortedReads[i + 1].mateIdx = i; ++i; }
  {
    const auto ts0 = std::chrono::steady_clock::now();
    sortReadsOnThreads(sortedReads, threadCnt, [](const SortRead &a, const SortRead &b) { return a < b; }, true, &sortSpare);
    if (!hasBarcode) std::vector<SortRead>().swap(sortSpare);   // (only barcode mode sorts again)
    if (getenv("T4_TIMING")) PrintLog("timing: read list sorted in %.2f s on %d threads", std::chrono::duration<double>(std::chrono::steady_clock::now() - ts0).count(), threadCnt);
  }
  mark("sorted");
  PrintLog("Finish sorting the reads.");

  // ---- rough annotation on the GPU (main.cpp:1084-1120): every distinct read once, in chunks (a 20 M-pair input must not need
  // all packed reads and all 160-byte results at the same time)
  {
    const size_t CHUNK = getenv("T4_ANNOT_CHUNK") && atoll(getenv("T4_ANNOT_CHUNK")) > 0 ? (size_t)atoll(getenv("T4_ANNOT_CHUNK")) : (size_t)4 << 20;   // distinct reads per t4_annotate_rough call (the variable: a testing aid, small inputs through many chunks)
    std::string &bases = scratchBases; std::vector<int64_t> &off = scratchOff; std::vector<int> firstOf; std::vector<t4_overlap> out;
    // --readShard R/N (bulk mode: "the read-only passes shard by read range, index replicated, no exchange except gathering
    // 128-B results"): this process annotates the R-th of N ranges of read positions (cut where a new distinct read starts)
    int sliceLo = 0, sliceHi = readCnt;
    if (annotCount > 1) {
      auto cut = [&](int r) { long long p = (long long)readCnt * r / annotCount; while (p > 0 && p < readCnt && sortedReads[(size_t)p].read == sortedReads[(size_t)p - 1].read) ++p; return (int)(p > readCnt ? readCnt : p); };
      sliceLo = cut(annotRank); sliceHi = cut(annotRank + 1);
    }
    int i = sliceLo;
    while (i < sliceHi) {
      firstOf.clear();
      const int chunkBegin = i;
      {   // the first positions of the chunk's distinct reads: the comparisons on the threads, the walk over their flags serial
        const int span = (int)((long long)sliceHi - i < (long long)CHUNK * 4 ? sliceHi - i : CHUNK * 4);
        std::vector<unsigned char> isFirst((size_t)span);
        parallelFor((long long)span, threadCnt, [&](long long d) { const int t = chunkBegin + (int)d; isFirst[(size_t)d] = t == 0 || sortedReads[(size_t)t].read != sortedReads[(size_t)t - 1].read; });
        int d = 0;
        for (; d < span && firstOf.size() < CHUNK; ++d) if (isFirst[(size_t)d]) firstOf.push_back(chunkBegin + d);
        while (d < span && !isFirst[(size_t)d]) ++d;   // the copies of the chunk's last read belong to it
        i = chunkBegin + d;
        if (d == span) while (i < sliceHi && sortedReads[(size_t)i].read == sortedReads[(size_t)i - 1].read) ++i;
      }
      const int n = (int)firstOf.size();
      if (n == 0) break;
      off.resize((size_t)n + 1); off[0] = 0;
      for (int k = 0; k < n; ++k) off[(size_t)k + 1] = off[(size_t)k] + (int64_t)sortedReads[(size_t)firstOf[(size_t)k]].read.size();
      bases.resize((size_t)off[(size_t)n]);
      parallelFor((long long)n, threadCnt, [&](long long k) { const std::string &r = sortedReads[(size_t)firstOf[(size_t)k]].read; if (!r.empty()) memcpy(&bases[(size_t)off[(size_t)k]], r.data(), r.size()); });
      t4_batch *batch = nullptr;
      if ((rc = t4_reads_upload(ctx, bases.data(), off.data(), nullptr, n, &batch))) die(ctx, "t4_reads_upload", rc);
      out.resize(4 * (size_t)n);
      if ((rc = t4_annotate_rough(refSet, batch, out.data()))) die(ctx, "t4_annotate_rough", rc);
      { t4_stats st; if (t4_last_stats(ctx, &st) == T4_OK) { annotKernelMs += st.chain_kernel_ms; annotHits += st.total_hits; annotReads += st.reads; } }
      t4_batch_destroy(batch);
      parallelFor((long long)n, threadCnt, [&](long long k) {   // every copy of a read takes its annotation
        const int tEnd = k + 1 < n ? firstOf[(size_t)k + 1] : i;
        for (int t = firstOf[(size_t)k]; t < tEnd; ++t) for (int j = 0; j < 4; ++j) sortedReads[(size_t)t].g[j] = out[4 * (size_t)k + j];
      });
    }
    if (annotSharded) {   // (with N = 1 too: one rank still runs every call of the exchange)
      // the one exchange of this mode: every rank's annotation records (4 x 40 bytes per read position of its range) to every rank --
      // RCCL all-gather on the ctx's stream (t4_comm) or files of a shared directory; the ranges are known to all, so no header travels
      std::string mine((size_t)(sliceHi - sliceLo) * 4 * sizeof(t4_overlap), '\0');
      for (int t = sliceLo; t < sliceHi; ++t) memcpy(&mine[(size_t)(t - sliceLo) * 4 * sizeof(t4_overlap)], sortedReads[(size_t)t].g, 4 * sizeof(t4_overlap));
      std::vector<std::string> got((size_t)annotCount);
      if (gatherDir.empty()) (void)commUp(annotRank, annotCount, rcclIdPath);   // (falls back to files on every rank alike)
      if (!gatherDir.empty()) {
        const std::string mineP = gatherDir + "/annot.rank" + std::to_string(annotRank);
        FILE *fp = fopen((mineP + ".tmp").c_str(), "wb");
        if (!fp || fwrite(mine.data(), 1, mine.size(), fp) != mine.size()) { fprintf(stderr, "trust4-hip: cannot write %s\n", mineP.c_str()); return EXIT_FAILURE; }
        fclose(fp);
        if (rename((mineP + ".tmp").c_str(), mineP.c_str())) { fprintf(stderr, "trust4-hip: cannot create %s\n", mineP.c_str()); return EXIT_FAILURE; }
        for (int r = 0; r < annotCount; ++r) {
          if (r == annotRank) { got[(size_t)r] = mine; continue; }
          bool ok = false;
          for (int tries = 0; tries < 36000 && !ok; ++tries) {
            FILE *fq = fopen((gatherDir + "/annot.rank" + std::to_string(r)).c_str(), "rb");
            if (fq) { char buf[1 << 16]; size_t nr; std::string &dst = got[(size_t)r]; dst.clear(); while ((nr = fread(buf, 1, sizeof buf, fq)) > 0) dst.append(buf, nr); fclose(fq); ok = true; }
            else usleep(50000);
          }
          if (!ok) { fprintf(stderr, "trust4-hip: no annotations from rank %d in %s\n", r, gatherDir.c_str()); return EXIT_FAILURE; }
        }
      } else {
        void *all = nullptr;
        std::vector<int64_t> sizes((size_t)annotCount);
        if ((rc = t4_comm_allgather_bytes(comm, mine.data(), (int64_t)mine.size(), &all, sizes.data()))) die(ctx, "t4_comm_allgather_bytes", rc);
        size_t at = 0;
        for (int r = 0; r < annotCount; ++r) { got[(size_t)r].assign((const char *)all + at, (size_t)sizes[(size_t)r]); at += (size_t)sizes[(size_t)r]; }
        free(all);
        t4_comm_destroy(comm); comm = nullptr;
      }
      for (int r = 0; r < annotCount; ++r) {
        auto cut = [&](int q) { long long p = (long long)readCnt * q / annotCount; while (p > 0 && p < readCnt && sortedReads[(size_t)p].read == sortedReads[(size_t)p - 1].read) ++p; return (int)(p > readCnt ? readCnt : p); };
        const int lo = cut(r), hi = cut(r + 1);
        if (got[(size_t)r].size() != (size_t)(hi - lo) * 4 * sizeof(t4_overlap)) { fprintf(stderr, "trust4-hip: rank %d sent %zu bytes of annotations, expected %zu\n", r, got[(size_t)r].size(), (size_t)(hi - lo) * 4 * sizeof(t4_overlap)); return EXIT_FAILURE; }
        if (r != annotRank) for (int t = lo; t < hi; ++t) memcpy(sortedReads[(size_t)t].g, &got[(size_t)r][(size_t)(t - lo) * 4 * sizeof(t4_overlap)], 4 * sizeof(t4_overlap));
      }
      PrintLog("Rough annotations of %d read ranges exchanged over %s (this rank: reads %d-%d of %d).", annotCount, gatherDir.empty() ? "RCCL" : "files", sliceLo, sliceHi, readCnt);
      // (every rank has read every status by now -- nobody contributes to the exchange before -- so this rank's can go: ADVICE r5)
      if (!rcclIdPath.empty()) (void)unlink((rcclIdPath + ".status.rank" + std::to_string(annotRank)).c_str());
      if (annotRank != 0) {   // the ordered assembly pass is one chain: rank 0 runs it and writes the files
        t4_index_destroy(refSet);
        t4_destroy(ctx);
        return 0;
      }
    }
  }
  mark("rough_annotation");
  PrintLog("Finish rough annotations.");

  // ---- barcode order: by barcode, then by the barcode-wise 21-mer support (main.cpp:1123-1193)
  if (hasBarcode) {
    {   // compReadWithBarcode (main.cpp:128-136) is not a strict weak order once a read without barcode stands beside barcoded ones
      bool allBarcoded = true;
      for (const SortRead &r : sortedReads) if (r.barcode == -1) { allBarcoded = false; break; }
      sortReadsOnThreads(sortedReads, threadCnt, compReadWithBarcode, allBarcoded, &sortSpare);
      std::vector<SortRead>().swap(sortSpare);
    }
    PrintLog("Get barcode-wise kmer count.");
    std::vector<std::pair<int, int>> groups;
    for (int i = 0; i < readCnt;) {
      int j = i + 1;
      while (j < readCnt && sortedReads[j].barcode == sortedReads[i].barcode) ++j;
      groups.push_back({i, j});
      i = j;
    }
    // barcodes are numbered in order of appearance and a device table keys -1..T4_KMER_COUNT_MAX_BARCODE: a run with more of them counts
    // on the host (t4_kmer_count_add would refuse its batches)
    int maxBarcode = -1;
    for (const SortRead &r : sortedReads) if (r.barcode > maxBarcode) maxBarcode = r.barcode;
    const bool barcodesFit = maxBarcode <= T4_KMER_COUNT_MAX_BARCODE;
    if (gpuKmerCounts && !barcodesFit)
      PrintLog("Barcode-wise kmer count on the host threads: barcode %d is beyond the %d that the device table keys.", maxBarcode, T4_KMER_COUNT_MAX_BARCODE);
    if (gpuKmerCounts && barcodesFit) {   // one device table for all barcodes, the barcode being part of the key (t4_kmer_count_create, per_barcode)
      long long kmers = 0;
      for (const SortRead &r : sortedReads) if ((int)r.read.size() >= 21) kmers += (long long)r.read.size() - 20;
      t4_kmer_counter *bkc = nullptr;
      if ((rc = t4_kmer_count_create(ctx, 21, kmers + 16 < (1ll << 30) ? kmers + 16 : (1ll << 30), 1, &bkc))) die(ctx, "t4_kmer_count_create", rc);
      std::string &bases = scratchBases; std::vector<int64_t> &off = scratchOff;
      std::vector<int32_t> mn, md, nl; std::vector<float> av;
      const bool keep = sortedReads.size() <= ((size_t)16 << 20);   // the chunks of the count pass serve the statistics pass (nothing changes in between)
      std::vector<t4_batch *> kept;
      for (int pass = 0; pass < 2; ++pass)
        for (size_t lo = 0, ci = 0; lo < sortedReads.size(); lo += KC_CHUNK, ++ci) {
          const size_t hi = lo + KC_CHUNK < sortedReads.size() ? lo + KC_CHUNK : sortedReads.size(), n = hi - lo;
          t4_batch *b = pass == 1 && keep ? kept[ci] : uploadChunk(lo, hi, bases, off, true);
          if (pass == 0) { if ((rc = t4_kmer_count_add(bkc, b))) die(ctx, "t4_kmer_count_add", rc); }
          else {
            mn.resize(n); md.resize(n); nl.resize(n); av.resize(n);
            if ((rc = t4_kmer_count_stats(bkc, b, nullptr, nullptr, mn.data(), md.data(), av.data(), nl.data()))) die(ctx, "t4_kmer_count_stats", rc);
            parallelFor((long long)n, threadCnt, [&](long long i) { SortRead &r = sortedReads[lo + (size_t)i]; r.barcodeMinCnt = mn[(size_t)i]; r.barcodeMedianCnt = md[(size_t)i]; r.barcodeAvgCnt = av[(size_t)i]; });
          }
          if (pass == 0 && keep) kept.push_back(b); else t4_batch_destroy(b);
        }
      t4_kmer_count_destroy(bkc);
    } else
    parallelFor((long long)groups.size(), threadCnt, [&](long long gI) {   // one private counter per barcode
      const int i = groups[(size_t)gI].first, j = groups[(size_t)gI].second;
      KmerCounter bkc(21);
      bkc.maxReadLen = maxReadLen;
      for (int t = i; t < j; ++t) bkc.addCount(sortedReads[t].read);
      for (int t = i; t < j; ++t)
        bkc.statsAndTrim(sortedReads[t].read, nullptr, sortedReads[t].barcodeMinCnt, sortedReads[t].barcodeMedianCnt, sortedReads[t].barcodeAvgCnt);
    });
    PrintLog("Finish barcode-wise kmer count.");
    parallelFor((long long)groups.size(), threadCnt, [&](long long gI) {
      const int i = groups[(size_t)gI].first, j = groups[(size_t)gI].second;
      if (j - i > 1) std::sort(sortedReads.begin() + i, sortedReads.begin() + j, compReadWithBarcode);
    });
    PrintLog("Finish re-sorting the reads based on barcode.");
  }

  // ---- mate links in sorted order, V / C trimming (main.cpp:1208-1526)
  std::vector<int> originToSorted(readCnt);
  std::vector<char> goodCandidate(readCnt, 0);
  for (int i = 0; i < readCnt; ++i) originToSorted[sortedReads[i].info] = i;
  for (int i = 0; i < readCnt; ++i) if (sortedReads[i].mateIdx != -1) sortedReads[i].mateIdx = originToSorted[sortedReads[i].mateIdx];
  if (trimLevel > 1 && !hasBarcode) {   // the V gene assignment serves as a barcode (main.cpp:1224-1236)
    for (int i = 0; i < readCnt; ++i)
      if (sortedReads[i].g[0].seqIdx != -1 && sortedReads[i].g[0].similarity > 0.95) {
        sortedReads[i].barcode = sortedReads[i].g[0].seqIdx;
        if (sortedReads[i].mateIdx != -1) sortedReads[sortedReads[i].mateIdx].barcode = sortedReads[i].g[0].seqIdx;
      }
  }
  auto refName = [&](int idx) { return t4_index_seq_name(refSet, idx); };
  auto eraseFront = [](std::string &s, int n) { s.erase(0, n); };
  parallelFor((long long)readCnt, threadCnt, [&](long long i) {   // bases before the V gene (every read by itself: on the threads)
    SortRead &sr = sortedReads[(size_t)i];
    t4_overlap *g = sr.g;
    if (sr.dead || g[0].seqIdx == -1) return;
    bool mayTrim = false;
    if (g[0].seqStart < 31 && g[0].similarity > 0.9) mayTrim = true;
    if (g[0].similarity > 0.95 && g[0].seqStart <= t4_index_seq_len(refSet, g[0].seqIdx) / 3) mayTrim = true;
    if (trimLevel > 1) mayTrim = true;
    if (!mayTrim) return;
    int trimBase = g[0].readStart;
    if (trimLevel > 1 && refName(g[0].seqIdx)[0] == 'T' && g[0].similarity < 0.97) trimBase = (g[0].readStart + g[0].readEnd) / 2;
    if (trimBase <= 0) return;
    if (g[2].seqIdx != -1 && g[2].readStart < trimBase && trimLevel <= 1) return;
    if (g[3].seqIdx != -1 && g[3].readStart < trimBase && trimLevel <= 1) return;
    if (sr.len - trimBase < 31) { sr.dead = true; return; }
    if (g[0].strand >= 0) eraseFront(sr.read, trimBase); else sr.read.resize(sr.len - trimBase);
    for (int j = 0; j < 4; ++j) {
      if (g[j].seqIdx == -1) continue;
      g[j].readStart -= trimBase; g[j].readEnd -= trimBase;
      if (g[j].readStart < 0) g[j].readStart = 0;
      if (g[j].readEnd < 0) { g[j].readEnd = 0; g[j].seqIdx = -1; }
    }
    sr.len -= trimBase;
  });
  parallelFor((long long)readCnt, threadCnt, [&](long long i) {   // bases after the C gene (every read by itself: on the threads)
    SortRead &sr = sortedReads[(size_t)i];
    t4_overlap *g = sr.g;
    const int len = sr.len;
    if (sr.dead) return;
    int gidx;
    for (gidx = 2; gidx <= 3; ++gidx) if (g[gidx].seqIdx != -1) break;
    if (gidx > 3) return;
    if (gidx == 2 && refName(g[gidx].seqIdx)[2] == 'H') { gidx = 3; if (g[gidx].seqIdx == -1) return; }
    bool mayTrim = false;
    if (gidx == 3 && g[3].seqStart < 9 && g[3].similarity > 0.95) mayTrim = true;
    if (trimLevel > 1) mayTrim = true;
    if (!mayTrim) return;
    int trimBase = len - g[gidx].readEnd - 1;
    if (trimLevel > 1 && refName(g[gidx].seqIdx)[0] == 'T' && g[gidx].similarity < 0.97) trimBase = len - ((g[gidx].readStart + g[gidx].readEnd) / 2) - 1;
    if (trimBase <= 0) return;
    if (gidx == 3 && g[2].seqIdx != -1 && g[2].readStart + trimBase >= sr.len && trimLevel <= 1) return;
    if (g[0].seqIdx != -1 && g[0].readStart + trimBase >= sr.len && trimLevel <= 1) return;
    if (sr.len - trimBase < 31) { sr.dead = true; return; }
    if (g[gidx].strand < 0) eraseFront(sr.read, trimBase); else sr.read.resize(len - trimBase);
    g[3].seqIdx = -1;
    for (int j = 0; j < 4; ++j) {
      if (g[j].seqIdx == -1) continue;
      if (g[j].readStart + trimBase >= len) { g[j].readStart = len - 1; g[j].seqIdx = -1; }
      if (g[j].readEnd + trimBase >= len) g[j].readEnd = len - 1;
    }
    sr.len -= trimBase;
  });
  if (firstReadLen > 200) { fprintf(stderr, "trust4-hip: long-read mode (first read > 200 bp) is not built.\n"); return EXIT_FAILURE; }
  {
    std::vector<int> remap(readCnt, -1);
    std::vector<SortRead> kept;
    for (int i = 0; i < readCnt; ++i) if (!sortedReads[i].dead) { remap[i] = (int)kept.size(); kept.push_back(std::move(sortedReads[i])); }
    for (SortRead &r : kept) if (r.mateIdx != -1) r.mateIdx = remap[r.mateIdx];
    std::vector<char> gc(kept.size(), 0);
    sortedReads.swap(kept); goodCandidate.swap(gc);
    readCnt = (int)sortedReads.size();
  }

  // ---- the assembly loop (main.cpp:1528-1880)
  t4_assembler *seqSet = nullptr;     // bulk mode: the one contig set
  t4_cellset *cellSet = nullptr;      // barcode mode: one contig set per cell
  std::vector<t4_cellset *> cellSets;   // ... in groups of cells (cellSet = the first)
  std::vector<t4_ctx *> cellCtxs;
  int hitLenRequired = 31;
  if (firstReadLen / 2 < 31) { int l = firstReadLen / 2; if (l < 21) l = 21; hitLenRequired = l; }
  if (hasBarcode) hitLenRequired = 13;
  if (minHitLen != -1) hitLenRequired = minHitLen;
  int cellImageForm = T4_CELL_IMAGE_COMPACT;
  const char *const cellImageFormNames[] = {"compact", "indexed", "resident"};
  const bool useCells = hasBarcode && !keepMissingBarcode;   // --keepNoBarcode: the index is not keyed by barcode, one set
  if (useCells) {
    if (barcodeIntToStr.size() >= 1000003) { fprintf(stderr, "trust4-hip: more than 1000002 barcodes are not supported.\n"); return EXIT_FAILURE; }
    // Cells are independent, so the cells of this process are dealt to GROUPS contiguous groups, each with its own t4_ctx (stream,
    // scratch), t4_cellset (arena of cell images) and host thread: while one group's query batch runs on the GPU the others stage
    // images, collect and commit (round 4; one group = the round-3 loop: collect -> stage -> query -> commit, nothing overlapped).
    int G = getenv("T4_CELL_GROUPS") ? atoi(getenv("T4_CELL_GROUPS")) : (threadCnt >= 8 ? 4 : 2);   // (two even at -t 1: a group's thread mostly waits for its batch, like the reader threads it is not counted against -t)
    if (G < 1) G = 1;
    if (G > 16) G = 16;
    // (every group beyond the first costs the device a ctx of its own -- stream, scratch, result pools, an arena of cell images: a few
    // hundred MB --; on a shared or smaller GPU one that cannot be had is left out and the run goes on with the groups it has: one group
    // is the round-3 path. ADVICE r4.)
    cellCtxs.clear(); cellSets.clear();
    for (int g = 0; g < G; ++g) {
      t4_ctx *gc = ctx;
      t4_cellset *gs = nullptr;
      if (g > 0 && (rc = t4_init(getenv("T4_DEVICE") ? atoi(getenv("T4_DEVICE")) : 0, &gc))) { fprintf(stderr, "trust4-hip: no ctx for cell group %d (%d): going on with %d group(s)\n", g, rc, g); break; }
      if ((rc = t4_cellset_create(gc, indexKmerLength, &gs))) {
        if (g == 0) die(gc, "t4_cellset_create", rc);
        fprintf(stderr, "trust4-hip: no cell set for cell group %d (%s): going on with %d group(s)\n", g, t4_last_error(gc), g);
        t4_destroy(gc);
        break;
      }
      cellCtxs.push_back(gc); cellSets.push_back(gs);
    }
    G = (int)cellSets.size();
    // T4_CELL_IMAGES=indexed: the cells' images travel without their index, which the device builds from the contigs
    // T4_CELL_IMAGES=resident: the images stay in their slots, a change travels as the contigs it touched
    { const char *form = getenv("T4_CELL_IMAGES"); cellImageForm = form && !strcmp(form, "indexed") ? T4_CELL_IMAGE_INDEXED : form && !strcmp(form, "resident") ? T4_CELL_IMAGE_RESIDENT : T4_CELL_IMAGE_COMPACT; }
    if (getenv("T4_TIMING")) fprintf(stderr, "trust4-hip: cell images in the %s form\n", cellImageFormNames[cellImageForm]);
    for (int g = 0; g < G; ++g) {
      if (cellImageForm != T4_CELL_IMAGE_COMPACT && (rc = t4_cellset_set_image_form(cellSets[(size_t)g], cellImageForm))) die(cellCtxs[(size_t)g], "t4_cellset_set_image_form", rc);
      t4_cellset_set_params(cellSets[(size_t)g], hitLenRequired, 10, 0.9);
      t4_cellset_set_threads(cellSets[(size_t)g], (threadCnt + G - 1) / G);
    }
    cellSet = cellSets[0];
  } else {
    if ((rc = t4_assembler_create(ctx, indexKmerLength, 0, &seqSet))) die(ctx, "t4_assembler_create", rc);
    t4_assembler_set_params(seqSet, hitLenRequired, 10, 0.9);
    // (the helpers beside the chain's host thread: dependency records and window k-mers of a round's fresh reads, a few hundred
    // microseconds of work per round -- more than eight of them cost more in wake-ups than they take off it: C2 67 s at -t 16 / 32 against
    // 61 s at -t 8 in round 5; the input phases take all of -t)
    t4_assembler_set_threads(seqSet, getenv("T4_CHAIN_THREADS") ? atoi(getenv("T4_CHAIN_THREADS")) > 0 ? atoi(getenv("T4_CHAIN_THREADS")) : 1 : (threadCnt < 8 ? threadCnt : 8));
  }
  for (const NovelFa &nf : novelFa) {   // SeqSet::InputNovelFa (SeqSet.hpp:2986-2993): every record becomes a contig, strand 1, no barcode
    if (useCells) { fprintf(stderr, "trust4-hip: --debug-ns is not supported together with --barcode (use --keepNoBarcode).\n"); return EXIT_FAILURE; }
    SeqReader fa;
    fa.files.push_back(nf.file);
    while (fa.next())
      if ((rc = t4_assembler_input_novel_read(seqSet, fa.id.c_str(), fa.seq.c_str(), 1, -1)) < 0) die(ctx, "t4_assembler_input_novel_read", rc);
  }
  if (trimLevel > 1) changeKmerLengthThreshold /= 2;
  std::vector<int> barcodeTotalReadCount(barcodeIntToStr.size(), 0), barcodeReadCount(barcodeIntToStr.size(), 0);
  if (hasBarcode) for (int i = 0; i < readCnt; ++i) if (sortedReads[i].barcode != -1) ++barcodeTotalReadCount[sortedReads[i].barcode];
  std::atomic<int> assembledReadCnt(0);
  // upcoming AddRead reads queried per round: per cell in barcode mode (a cell's window ends at its first observable change);
  // in bulk mode the window slides and keeps what still stands, so it is as wide as one launch serves at single-read latency
  const int WINDOW = getenv("T4_WINDOW") ? atoi(getenv("T4_WINDOW")) : (hasBarcode && !keepMissingBarcode ? 4 : 192);
  const int LANES = getenv("T4_LANES") ? atoi(getenv("T4_LANES")) : 4096;

  // AddRead arguments of read i that do not depend on the loop state (main.cpp:1609-1701)
  struct AddArgs { bool filter; char name[5]; int strand; double thr; };
  auto addArgs = [&](int i) {
    AddArgs a; a.filter = false; a.name[0] = 0; a.strand = 0;
    const t4_overlap *g = sortedReads[i].g;
    for (int j = 0; j < 4 && !a.filter; ++j) {
      if (g[j].seqIdx == -1) continue;
      for (int l = j + 1; l < 4; ++l) { if (g[l].seqIdx == -1) continue; if (g[j].readEnd - 10 > g[l].readStart) { a.filter = true; break; } }
    }
    if (g[3].seqIdx != -1 && g[0].seqIdx == -1 && g[2].seqIdx == -1) {
      if (g[3].seqStart >= constantGeneEnd) a.filter = true;
      else if (constantGeneEnd <= 200 && g[3].seqStart >= 100 && (g[3].strand == 1 || g[3].readEnd - g[3].readStart + 1 < sortedReads[i].len)) a.filter = true;
    }
    int ambiguous = 0;
    for (int j = 0; j < 4; ++j)
      if (g[j].seqIdx != -1) {
        const char *s = refName(g[j].seqIdx);
        a.name[0] = s[0]; a.name[1] = s[1]; a.name[2] = s[2]; a.name[3] = s[3]; a.name[4] = 0;
        if (a.strand != 0 && a.strand != g[j].strand) ambiguous = 1;
        a.strand = g[j].strand;
      }
    if (ambiguous) a.strand = 0;
    a.thr = 0.9;
    if (sortedReads[i].minCnt >= 20) a.thr = 0.97; else if (sortedReads[i].minCnt >= 2) a.thr = 0.95;
    if (a.name[0] == 'T' && a.thr < 0.95) a.thr = 0.95;
    if (hasBarcode || trimLevel > 1) a.thr = 0.9;
    return a;
  };
  auto isNewRead = [&](int i) { return i == 0 || sortedReads[i].read != sortedReads[i - 1].read || sortedReads[i].barcode != sortedReads[i - 1].barcode; };
  std::vector<t4_assembler *> cellOf;   // barcode mode: the cell of every read this process assembles
  auto setOf = [&](int i) { return useCells ? cellOf[i] : seqSet; };

  // One walk = a run of consecutive reads processed in order: the whole input in bulk mode, one cell (or a chain of
  // cells whose boundary reads are identical, see below) in barcode mode.
  struct Walk {
    int begin = 0, end = 0, cur = 0, prevAddRet = -1;
    const t4_overlap *g = nullptr;   // the reference's `static geneOverlap[4]`: refreshed for new sequences only
    std::vector<int> rescue, assembledMain, assembledRescue;
    size_t rcur = 0;
    int phase = 0;   // 0 main pass, 1 rescue pass, 2 done
  };
  auto needsQuery = [&](int i) { return isNewRead(i) && !addArgs(i).filter; };

  // main.cpp:1585-1870 for read w.cur
  auto stepMain = [&](Walk &w) {
    const int i = w.cur;
    t4_assembler *set = setOf(i);
    const int barcode = sortedReads[i].barcode;
    int addRet = -1;
    if (isNewRead(i)) {
      w.g = sortedReads[i].g;
      const t4_overlap *g = w.g;
      AddArgs a = addArgs(i);
      if (!a.filter) {
        int strand = a.strand;
        const int minKmerCount = hasBarcode ? (sortedReads[i].minCnt + sortedReads[i].barcodeMinCnt + 1) / 2 : sortedReads[i].minCnt;
        addRet = t4_assembler_add_read(set, sortedReads[i].read.c_str(), a.name, &strand, barcode, minKmerCount, trimLevel > 1, a.thr);
        if (addRet < -50) die(ctx, "t4_assembler_add_read", addRet + 100);
        if (addRet < 0) {
          int matchCnt = 0;
          for (int j = 0; j < 4; ++j) if (g[j].seqIdx != -1) matchCnt += g[j].matchCnt / 2;
          bool filter = true;
          if (matchCnt >= 31) filter = false;
          else if (g[0].seqIdx != -1 && g[2].seqIdx != -1 && g[0].readEnd < g[2].readStart) filter = false;
          else if (g[0].seqIdx != -1) { if (g[0].seqEnd >= t4_index_seq_len(refSet, g[0].seqIdx) - 17) filter = false; }
          else if (g[2].seqIdx != -1) { if (g[2].seqStart <= 17) filter = false; }
          int j;
          for (j = 0; j < 4; ++j) if (g[j].seqIdx != -1) break;
          if (!filter) addRet = t4_assembler_input_novel_read(set, refName(g[j].seqIdx), sortedReads[i].read.c_str(), g[j].strand, barcode);
          else if (goodCandidate[i]) {
            int ms = -sortedReads[sortedReads[i].info].strand;
            if (hasMotif(sortedReads[i].read, ms)) addRet = t4_assembler_input_novel_read(set, "Novel", sortedReads[i].read.c_str(), ms, barcode);
          }
        }
        sortedReads[i].strand = strand;
      }
    } else {
      if (w.prevAddRet != -1 && w.prevAddRet != -3) addRet = t4_assembler_repeat_add_read(set, sortedReads[i].read.c_str());
      else if (w.prevAddRet == -3) addRet = -3;
      sortedReads[i].strand = sortedReads[i - 1].strand;
    }
    const t4_overlap *g = w.g;
    if (addRet == -2) w.rescue.push_back(i);
    else if (addRet >= 0) {
      ++assembledReadCnt;
      w.assembledMain.push_back(i);
      if (sortedReads[i].mateIdx > i) {   // good-candidate propagation to the mate (main.cpp:1781-1843)
        bool good = false, maySpan = false;
        if (g[0].seqIdx != -1 && g[0].similarity >= 0.9 && sortedReads[i].strand == 1) {
          good = true;
          if (g[2].seqIdx != -1 && g[2].readStart > g[0].readEnd) maySpan = true;
          if (g[3].seqIdx != -1 && g[3].readStart > g[0].readEnd) maySpan = true;
        }
        for (int j = 2; j <= 3; ++j)
          if (g[j].seqIdx != -1 && g[j].similarity >= 0.9 && sortedReads[i].strand == -1) {
            good = true;
            if (g[0].seqIdx != -1 && g[j].readStart > g[0].readEnd) maySpan = true;
          }
        if (maySpan) good = false;
        const int tag = sortedReads[i].mateIdx;
        if (good && !goodCandidate[tag]) {   // the loops only compare sequences: they may run into the neighbouring cells
          for (int j = tag - 1; j > 0; --j) { if (sortedReads[j].read == sortedReads[tag].read) { goodCandidate[j] = 1; sortedReads[j].info = i; } else break; }
          for (int j = tag + 1; j < readCnt; ++j) { if (sortedReads[j].read == sortedReads[tag].read) { goodCandidate[j] = 1; sortedReads[j].info = i; } else break; }
        }
        if (good) { goodCandidate[tag] = 1; sortedReads[tag].info = i; }
      }
      if (useCells && barcode != -1) {   // a barcode whose every read was assembled leaves the index (main.cpp:1846-1859)
        if (++barcodeReadCount[barcode] >= barcodeTotalReadCount[barcode]) t4_assembler_release_finished_barcode(set, barcode, contigMinCov);
      }
    }
    w.prevAddRet = addRet;
    ++w.cur;
  };
  // main.cpp:1904-1937 for rescue read w.rescue[w.rcur]
  auto stepRescue = [&](Walk &w) {
    const int idx = w.rescue[w.rcur++];
    SortRead &sr = sortedReads[idx];
    double thr = 0.9;
    if (sr.minCnt >= 20) thr = 0.97; else if (sr.minCnt >= 2) thr = 0.95;
    int strand = 0;
    int addRet = t4_assembler_add_read(setOf(idx), sr.read.c_str(), "", &strand, sr.barcode, 1, trimLevel > 1, thr);
    if (addRet < -50) die(ctx, "t4_assembler_add_read", addRet + 100);
    sr.strand = strand;
    if (addRet >= 0) { ++assembledReadCnt; w.assembledRescue.push_back(idx); }
  };

  mark("trimmed_ready");
  if (getenv("T4_PHASE_DUMP")) t4_debug_phase_reset();
  std::vector<int> assembledReadIdx;
  int rescueReadCnt = 0, rescuedCnt = 0;
  int64_t laneBatches = 0, fallbackQueries = 0;
  if (!useCells) {
    Walk w;
    w.begin = 0; w.end = readCnt;
    // The reads that will be offered to AddRead with a query of their own (distinct, not filtered), in order, with the arguments they
    // will be offered with: none of it depends on the loop state (addArgs), so the list is made once, on the host threads -- the
    // announcement of a round is a slice of it (making it afresh every round cost the chain 60 us per round: 7 s of config C2)
    std::vector<int> qOf; std::vector<const char *> qReads; std::vector<int> qStrand, qBarcode;
    if (WINDOW > 1) {
      std::vector<unsigned char> isQ((size_t)readCnt, 0);
      std::vector<int> stOf((size_t)readCnt, 0);
      parallelFor((long long)readCnt, threadCnt, [&](long long j) {
        if (!isNewRead((int)j)) return;
        const AddArgs b = addArgs((int)j);
        if (b.filter) return;
        isQ[(size_t)j] = 1; stOf[(size_t)j] = b.strand;
      });
      for (int j = 0; j < readCnt; ++j) if (isQ[(size_t)j]) { qOf.push_back(j); qReads.push_back(sortedReads[j].read.c_str()); qStrand.push_back(stOf[(size_t)j]); qBarcode.push_back(sortedReads[j].barcode); }
    }
    size_t qPos = 0;
    while (w.cur < w.end) {
      const int i = w.cur;
      while (qPos < qOf.size() && qOf[qPos] < i) ++qPos;
      if (WINDOW > 1 && qPos < qOf.size() && qOf[qPos] == i && !t4_assembler_window_valid(seqSet)) {   // speculate on the next distinct, unfiltered reads
        const int n = (int)(qOf.size() - qPos < (size_t)WINDOW ? qOf.size() - qPos : (size_t)WINDOW);
        if ((rc = t4_assembler_prefetch(seqSet, n, qReads.data() + qPos, qStrand.data() + qPos, qBarcode.data() + qPos, trimLevel > 1))) die(ctx, "t4_assembler_prefetch", rc);
      }
      stepMain(w);
      if (assembledReadCnt > 0 && assembledReadCnt % 10000 == 0 && !hasBarcode) t4_assembler_update_all_consensus(seqSet);
      if ((i + 1) % 100000 == 0) PrintLog("Processed %d reads (%d are used for assembly).", i + 1, assembledReadCnt.load());
      if (t4_assembler_size(seqSet) > changeKmerLengthThreshold && indexKmerLength < 16 && !hasBarcode) {
        changeKmerLengthThreshold *= 4;
        indexKmerLength += 2;
        t4_assembler_change_kmer_length(seqSet, indexKmerLength);
      }
    }
    t4_assembler_update_all_consensus(seqSet);
    PrintLog("Assembled %d reads.", assembledReadCnt.load());
    rescueReadCnt = (int)w.rescue.size();
    PrintLog("Try to rescue %d reads for assembly.", rescueReadCnt);
    const int before = assembledReadCnt;
    while (w.rcur < w.rescue.size()) stepRescue(w);
    rescuedCnt = assembledReadCnt - before;
    t4_assembler_update_all_consensus(seqSet);
    PrintLog("Rescued %d reads.", rescuedCnt);
    assembledReadIdx = w.assembledMain;
    assembledReadIdx.insert(assembledReadIdx.end(), w.assembledRescue.begin(), w.assembledRescue.end());
  } else {
    // Cells are independent contig sets (see t4_cellset in trust4_hip.h), so the reference's cell-after-cell pass can be
    // replayed with many cells in flight: every round takes up to WINDOW upcoming AddRead reads of each active walk, queries
    // them all in one launch, then lets every walk commit its reads in order. Per cell the sequence of calls is the
    // reference's: main pass, UpdateAllConsensus, rescue reads, UpdateAllConsensus (main.cpp:1583-1940 with the passes of
    // different cells interleaved, which they cannot observe). One coupling exists: the good-candidate propagation compares
    // read sequences only and can cross into the next cell when the boundary reads are identical; such cells form one walk.
    std::vector<Walk> walks;
    for (int i = 0; i < readCnt;) {
      int j = i + 1;
      while (j < readCnt && (sortedReads[j].barcode == sortedReads[j - 1].barcode || sortedReads[j].read == sortedReads[j - 1].read)) ++j;
      Walk w; w.begin = w.cur = i; w.end = j;
      walks.push_back(w);
      i = j;
    }
    size_t firstWalk = 0, endWalkAll = walks.size();
    if (earlyShard) {
      // every read here is this rank's. The coupling of neighbouring cells -- a walk that runs on into the next cell because the reads
      // either side of the boundary are identical -- must not cross a rank boundary: the ranks tell each other their first and last read
      std::vector<std::string> ends;
      const std::string mineEnds = readCnt > 0 ? sortedReads[0].read + "\n" + sortedReads[(size_t)readCnt - 1].read : std::string();
      if (!exchange(mineEnds, true, ends)) { fprintf(stderr, "trust4-hip: the exchange of the boundary reads failed\n"); return EXIT_FAILURE; }
      bool coupled = testForceCoupled;   // (testing aid: the fallback below on inputs that do not need it)
      std::string lastSeen;
      for (int r = 0; r < shardCount; ++r) {
        if (ends[(size_t)r].empty()) continue;
        const size_t nl = ends[(size_t)r].find('\n');
        const std::string first = ends[(size_t)r].substr(0, nl), last = ends[(size_t)r].substr(nl + 1);
        if (!lastSeen.empty() && lastSeen == first) coupled = true;
        lastSeen = last;
      }
      if (coupled) {
        // rare (the last read of one rank's cells and the first read of the next rank's are the same sequence): the sample is run
        // again with every rank keeping all reads up to the cell pass, where whole walks are dealt out (--lateShard). The device is
        // given back first; the second attempt is a process of its own and this one passes its status on.
        PrintLog("Identical reads either side of a rank boundary: starting over with --lateShard.");
        if (comm) { t4_comm_destroy(comm); comm = nullptr; }
        for (size_t g = 0; g < cellSets.size(); ++g) { t4_cellset_destroy(cellSets[g]); if (g > 0) t4_destroy(cellCtxs[g]); }
        cellSets.clear();
        t4_index_destroy(refSet);
        t4_destroy(ctx);
        std::vector<SortRead>().swap(sortedReads);
        std::vector<char *> av2;
        for (int a = 0; a < argc; ++a) av2.push_back(argv[a]);
        char flag[] = "--lateShard";
        av2.push_back(flag); av2.push_back(nullptr);
        fflush(nullptr);
        pid_t child = 0;
        if (posix_spawn(&child, "/proc/self/exe", nullptr, nullptr, av2.data(), environ) != 0) { fprintf(stderr, "trust4-hip: cannot start the --lateShard run\n"); return EXIT_FAILURE; }
        int st = 0;
        if (waitpid(child, &st, 0) < 0) return EXIT_FAILURE;
        exit(WIFEXITED(st) ? WEXITSTATUS(st) : EXIT_FAILURE);
      }
    } else
    if (shardCount > 1) {   // (--lateShard) contiguous ranges of walks with about the same number of reads
      auto bound = [&](int r) {
        const long long target = (long long)readCnt * r / shardCount;
        size_t wI = 0;
        while (wI < walks.size() && walks[wI].begin < target) ++wI;
        return wI;
      };
      firstWalk = bound(shardRank); endWalkAll = bound(shardRank + 1);
    }
    // the walks of this process in G contiguous groups of about the same number of reads (contiguous: the output numbers the contigs
    // cell after cell, so a group's ids are its local ones + the contig slots of the groups before it)
    const int G = (int)cellSets.size();
    std::vector<size_t> groupBegin((size_t)G + 1, endWalkAll);
    {
      const long long lo = firstWalk < walks.size() ? walks[firstWalk].begin : readCnt, hi = endWalkAll < walks.size() ? walks[endWalkAll].begin : readCnt;
      size_t wI = firstWalk;
      for (int g = 0; g < G; ++g) {
        const long long target = lo + (hi - lo) * g / G;
        while (wI < endWalkAll && walks[wI].begin < target) ++wI;
        groupBegin[(size_t)g] = wI;
      }
    }
    cellOf.assign(readCnt, nullptr);
    for (int g = 0; g < G; ++g)
      for (size_t wI = groupBegin[(size_t)g]; wI < groupBegin[(size_t)g + 1]; ++wI)
        for (int i = walks[wI].begin; i < walks[wI].end; ++i) if ((rc = t4_cellset_cell(cellSets[(size_t)g], sortedReads[i].barcode, &cellOf[i]))) die(cellCtxs[(size_t)g], "t4_cellset_cell", rc);
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    auto finishMain = [&](Walk &w) {
      for (int i = w.begin; i < w.end; ++i) if (i == w.begin || cellOf[i] != cellOf[i - 1]) t4_assembler_update_all_consensus(cellOf[i]);
      w.phase = w.rescue.empty() ? 2 : 1;
    };
    struct GroupClock { double collect = 0, prefetch = 0, commit = 0, wall = 0; int64_t batches = 0; };
    std::vector<GroupClock> clocks((size_t)G);
    const int lanesOfGroup = LANES / G > 0 ? LANES / G : 1;
    const int commitThreads = (threadCnt + G - 1) / G;
    auto runGroup = [&](int g) {
    tlsErrCtx = cellCtxs[(size_t)g];
    t4_cellset *cellSet = cellSets[(size_t)g];
    t4_ctx *ctx = cellCtxs[(size_t)g];
    int rc = 0;
    GroupClock &clk = clocks[(size_t)g];
    const auto tg0 = now();
    size_t nextWalk = groupBegin[(size_t)g];
    const size_t endWalk = groupBegin[(size_t)g + 1];
    std::vector<int> active;
    auto cellsOfWalkDone = [&](Walk &w) {   // its cells will not be queried again
      for (int i = w.begin; i < w.end; ++i) if (i == w.begin || cellOf[i] != cellOf[i - 1]) t4_cellset_close_cell(cellSet, cellOf[i]);
    };
    while (nextWalk < endWalk || !active.empty()) {
      while (nextWalk < endWalk && (int)active.size() < lanesOfGroup) active.push_back((int)nextWalk++);
      // the upcoming AddRead reads of every active walk
      auto tc0 = now();
      std::vector<t4_assembler *> qc; std::vector<const char *> qr; std::vector<int> qs;
      std::vector<int> quota(active.size(), 0);
      for (size_t a = 0; a < active.size(); ++a) {
        Walk &w = walks[active[a]];
        if (w.phase == 0) {
          for (int j = w.cur; j < w.end && quota[a] < WINDOW; ++j) {
            if (!isNewRead(j)) continue;
            AddArgs b = addArgs(j);
            if (b.filter) continue;
            qc.push_back(cellOf[j]); qr.push_back(sortedReads[j].read.c_str()); qs.push_back(b.strand); ++quota[a];
          }
        } else {
          for (size_t j = w.rcur; j < w.rescue.size() && quota[a] < WINDOW; ++j) {
            qc.push_back(cellOf[w.rescue[j]]); qr.push_back(sortedReads[w.rescue[j]].read.c_str()); qs.push_back(0); ++quota[a];
          }
        }
      }
      clk.collect += since(tc0);
      auto tp0 = now();
      if (!qc.empty()) {
        if ((rc = t4_cellset_prefetch(cellSet, (int)qc.size(), qc.data(), qr.data(), qs.data(), trimLevel > 1))) die(ctx, "t4_cellset_prefetch", rc);
        ++clk.batches;
      }
      clk.prefetch += since(tp0);
      // commit, walk by walk, what was queried (reads that need no query ride along)
      auto tm0 = now();
      // walks own disjoint cells and disjoint ranges of sortedReads / goodCandidate / barcodeReadCount: they commit concurrently
      auto commitWalk = [&](size_t a) {
        Walk &w = walks[active[a]];
        int left = quota[a];
        if (w.phase == 0) {
          while (w.cur < w.end) {
            if (needsQuery(w.cur)) {   // never fall back to a one-read launch: a read whose cached query a commit invalidated waits for the next round
              if (left == 0 || !t4_assembler_window_valid(cellOf[w.cur])) break;
              --left;
            }
            stepMain(w);
          }
          if (w.cur >= w.end) finishMain(w);
        } else if (w.phase == 1) {
          while (w.rcur < w.rescue.size() && left > 0 && t4_assembler_window_valid(cellOf[w.rescue[w.rcur]])) { stepRescue(w); --left; }
          if (w.rcur >= w.rescue.size()) {
            for (int i = w.begin; i < w.end; ++i) if (i == w.begin || cellOf[i] != cellOf[i - 1]) t4_assembler_update_all_consensus(cellOf[i]);
            w.phase = 2;
          }
        }
      };
      {
        const int nA = (int)active.size();
        const int nT = commitThreads < nA / 4 ? commitThreads : (nA / 4 > 0 ? nA / 4 : 1);
        std::atomic<int> nextA(0);
        auto worker = [&]() { tlsErrCtx = ctx; for (;;) { int b = nextA.fetch_add(8); if (b >= nA) break; for (int a = b; a < b + 8 && a < nA; ++a) commitWalk((size_t)a); } };
        std::vector<std::thread> pool;
        for (int t = 1; t < nT; ++t) pool.emplace_back(worker);
        worker();
        for (auto &th : pool) th.join();
      }
      std::vector<int> still;
      for (size_t a = 0; a < active.size(); ++a) {
        Walk &w = walks[active[a]];
        if (w.phase == 2) cellsOfWalkDone(w);   // arena bookkeeping: serial
        else still.push_back(active[a]);
      }
      active.swap(still);
      clk.commit += since(tm0);
    }
    clk.wall = since(tg0);
    tlsErrCtx = nullptr;
    };
    if (G == 1) runGroup(0);
    else {
      std::vector<std::thread> groupThreads;
      for (int g = 1; g < G; ++g) groupThreads.emplace_back(runGroup, g);
      runGroup(0);
      for (auto &th : groupThreads) th.join();
    }
    double secCollect = 0, secPrefetch = 0, secCommit = 0, secGroup = 0;
    for (const GroupClock &c : clocks) { laneBatches += c.batches; secCollect += c.collect; secPrefetch += c.prefetch; secCommit += c.commit; if (c.wall > secGroup) secGroup = c.wall; }
    if (G > 1) PrintLog("Cell groups: %d (each its own stream, image arena and host thread; slowest group %.2f s; the seconds below are sums over the groups).", G, secGroup);
    PrintLog("Assembly rounds: %lld (collect %.2f s, query batches incl. image staging %.2f s, ordered commits %.2f s).", (long long)laneBatches, secCollect, secPrefetch, secCommit);
    int mainCnt = 0;
    for (Walk &w : walks) { assembledReadIdx.insert(assembledReadIdx.end(), w.assembledMain.begin(), w.assembledMain.end()); mainCnt += (int)w.assembledMain.size(); rescueReadCnt += (int)w.rescue.size(); }
    for (Walk &w : walks) { assembledReadIdx.insert(assembledReadIdx.end(), w.assembledRescue.begin(), w.assembledRescue.end()); rescuedCnt += (int)w.assembledRescue.size(); }
    PrintLog("Assembled %d reads.", mainCnt);
    PrintLog("Try to rescue %d reads for assembly.", rescueReadCnt);
    PrintLog("Rescued %d reads.", rescuedCnt);
  }

  mark("assembled");
  // ---- outputs (main.cpp:1959-2036)
  std::vector<const char *> bnames;
  for (const std::string &b : barcodeIntToStr) bnames.push_back(b.c_str());
  // (returns the status instead of ending the process: two of these run on threads of their own below, and a die() there would call
  // exit() while the main thread is still writing the reads -- ADVICE r4; every caller reports after its join)
  auto writeSetRc = [&](const std::string &path, t4_ctx **errCtx, const char **what) -> int {
    int wrc = 0;
    if (useCells) {   // group after group: a group's contig ids follow the contig slots of the groups before it
      int base = 0;
      for (size_t g = 0; g < cellSets.size(); ++g) {
        if ((wrc = t4_cellset_output_at(cellSets[g], path.c_str(), bnames.data(), (int)bnames.size(), base, g > 0))) { *errCtx = cellCtxs[g]; *what = "t4_cellset_output_at"; return wrc; }
        base += t4_cellset_size(cellSets[g]);
      }
    }
    else if (hasBarcode) { if ((wrc = t4_assembler_output_barcodes(seqSet, path.c_str(), bnames.data(), (int)bnames.size()))) { *errCtx = ctx; *what = "t4_assembler_output_barcodes"; } }
    else if ((wrc = t4_assembler_output(seqSet, path.c_str()))) { *errCtx = ctx; *what = "t4_assembler_output"; }
    return wrc;
  };
  auto writeSet = [&](const std::string &path) {
    t4_ctx *ec = ctx; const char *what = "";
    const int wrc = writeSetRc(path, &ec, &what);
    if (wrc) die(ec, what, wrc);
  };
  if (contigMinCov > 0) {   // main.cpp:1952-1955
    if (useCells) { for (t4_cellset *cs : cellSets) t4_cellset_release_shallow_contigs(cs, contigMinCov); } else t4_assembler_release_shallow_contigs(seqSet, contigMinCov);
  }
  // a prefix starting with '-' sends the two contig files to stdout (main.cpp:1960-1966, 2021-2027)
  const bool toStdout = !outputPrefix.empty() && outputPrefix[0] == '-';
  auto writeSetOrStdout = [&](const std::string &path) {
    if (!toStdout) { writeSet(path); return; }
    char tmpl[] = "/tmp/trust4hip_XXXXXX";
    int fd = mkstemp(tmpl);
    if (fd < 0) { fprintf(stderr, "trust4-hip: cannot create a temporary file\n"); exit(EXIT_FAILURE); }
    close(fd);
    writeSet(tmpl);
    FILE *fp = fopen(tmpl, "r");
    char buf[65536];
    size_t n;
    while (fp && (n = fread(buf, 1, sizeof(buf), fp)) > 0) fwrite(buf, 1, n, stdout);
    if (fp) fclose(fp);
    fflush(stdout);
    unlink(tmpl);
  };
  // the records of _assembled_reads.fa (main.cpp:2011-2014) for positions [lo, hi) of assembledReadIdx: formatted on the threads, piece
  // after piece of the list, the pieces then joined or written in order
  auto formatReads = [&](size_t lo, size_t hi, const std::function<void(const std::string &)> &sink) {
    const size_t PIECE = 16384;
    const size_t nPieces = (hi - lo + PIECE - 1) / PIECE;
    const size_t WAVE = (size_t)(threadCnt > 1 ? threadCnt : 1) * 4;   // pieces formatted at a time (bounds the text held in memory)
    std::vector<std::string> text(WAVE);
    for (size_t p0 = 0; p0 < nPieces; p0 += WAVE) {
      const size_t np = nPieces - p0 < WAVE ? nPieces - p0 : WAVE;
      parallelFor((long long)np, threadCnt, [&](long long q) {
        std::string &t = text[(size_t)q];
        t.clear();
        const size_t a = lo + (p0 + (size_t)q) * PIECE, b = a + PIECE < hi ? a + PIECE : hi;
        char num[64];
        for (size_t w = a; w < b; ++w) {
          const SortRead &sr = sortedReads[(size_t)assembledReadIdx[w]];
          t += '>'; t += sr.id;
          t.append(num, (size_t)snprintf(num, sizeof num, " %d %d %d", sr.strand, sr.minCnt, sr.medianCnt));
          if (hasBarcode) { t += " barcode:"; t += barcodeIntToStr[(size_t)sr.barcode]; }
          if (hasUmi) t.append(num, (size_t)snprintf(num, sizeof num, " umi:%d", sr.umi));
          t += '\n'; t += sr.read; t += '\n';
        }
      });
      for (size_t q = 0; q < np; ++q) sink(text[q]);
    }
  };
  auto cellSlots = [&]() { int n = 0; for (t4_cellset *cs : cellSets) n += t4_cellset_size(cs); return n; };
  auto destroyCells = [&]() { for (size_t g = 0; g < cellSets.size(); ++g) { t4_cellset_destroy(cellSets[g]); if (g > 0) t4_destroy(cellCtxs[g]); } cellSets.clear(); };
  auto writeCellStats = [&]() {
    int64_t qb = 0, rq = 0, im = 0, by = 0, built = 0, keyRecs = 0, tabBytes = 0, indexed = 0, cntBytes = 0, postBuilt = 0, resWhole = 0, resDeltas = 0, resContigs = 0, resRestages = 0, resPost = 0, resTabBytes = 0, idxTabBytes = 0; double sq = 0, ss = 0;
    for (t4_cellset *cs : cellSets) {   // counts: sums over the cell groups; seconds: sums too (the groups overlap in time)
      int64_t a = 0, b = 0, c = 0, d = 0; double e = 0, f = 0;
      t4_cellset_counters(cs, &a, &b, &c, &d, &e, &f);
      qb += a; rq += b; im += c; by += d; sq += e; ss += f;
      int64_t is[4] = {0, 0, 0, 0};
      t4_cellset_image_stats(cs, is, 4);
      built += is[0]; keyRecs += is[1]; tabBytes += is[2];
      int64_t xs[4] = {0, 0, 0, 0};
      t4_cellset_indexed_stats(cs, xs, 4);
      indexed += xs[0]; cntBytes += xs[1]; postBuilt += xs[2]; idxTabBytes += xs[3];
      int64_t rs[7] = {0, 0, 0, 0, 0, 0, 0};
      t4_cellset_resident_stats(cs, rs, 7);
      resWhole += rs[0]; resDeltas += rs[1]; resContigs += rs[2]; resRestages += rs[4]; resPost += rs[5]; resTabBytes += rs[6];
    }
    if (const char *sj = getenv("T4_STATS_JSON")) {
      FILE *fp = fopen(sj, "w");
      if (fp) {
        fprintf(fp, "{\"reads\": %d, \"threads\": %d, \"phases_s\": {", readCnt, threadCnt);
        for (size_t i = 0; i < phaseMarks.size(); ++i) fprintf(fp, "%s\"%s\": %.4f", i ? ", " : "", phaseMarks[i].first.c_str(), phaseMarks[i].second);
        fprintf(fp, "}, \"rough_annotation\": {\"reads\": %lld, \"hits\": %lld, \"kernel_ms\": %.3f}, ", annotReads, annotHits, annotKernelMs);
        fprintf(fp, "\"cells\": {\"groups\": %d, \"query_batches\": %lld, \"reads_queried\": %lld, \"images_staged\": %lld, \"bytes_staged\": %lld, \"query_wall_s\": %.3f, \"stage_wall_s\": %.3f, "
                    "\"images_built_on_device\": %lld, \"key_records_shipped\": %lld, \"table_bytes_built_on_device\": %lld, "
                    "\"image_form\": \"%s\", \"images_indexed_on_device\": %lld, \"count_bytes_shipped\": %lld, \"postings_built_on_device\": %lld, "
                    "\"images_resident_whole\": %lld, \"deltas\": %lld, \"delta_contigs_shipped\": %lld, \"whole_restages\": %lld, "
                    "\"table_bytes_indexed_on_device\": %lld, \"postings_rebuilt_on_device\": %lld, \"table_bytes_rebuilt_on_device\": %lld}, ",
                (int)cellSets.size(), (long long)qb, (long long)rq, (long long)im, (long long)by, sq, ss, (long long)built, (long long)keyRecs, (long long)tabBytes,
                cellImageFormNames[cellImageForm], (long long)indexed, (long long)cntBytes, (long long)postBuilt,
                (long long)resWhole, (long long)resDeltas, (long long)resContigs, (long long)resRestages,
                (long long)idxTabBytes, (long long)resPost, (long long)resTabBytes);
        fprintf(fp, "\"contigs\": %d, \"assembled_reads\": %d}\n", cellSlots(), (int)assembledReadIdx.size());
        fclose(fp);
      }
    }
    PrintLog("Finish assembly. (%lld cells; GPU query batches %lld with %lld reads in %.2f s; %lld cell images, %.1f MB, staged in %.2f s)",
             (long long)barcodeIntToStr.size(), (long long)qb, (long long)rq, sq, (long long)im, by / 1e6, ss);
  };
  if (!annotSharded && (!rcclIdPath.empty() || !gatherDir.empty())) {
    // ---- the one exchange of barcode mode, inside the engine. Every rank holds the contig records of its cells (ids local to the
    // shard) and its assembled reads. (1) a small all-gather: contig slots and byte counts of every rank; (2) every rank renumbers
    // ITS OWN records as the reference's cell-after-cell pass numbers them (id += the slots of the earlier ranks); (3) the renumbered
    // records are gathered to rank 0, which writes _raw.out / _final.out; (4) every rank writes its own slice of
    // _assembled_reads.fa at the offset the byte counts give it -- the read texts (the bulk of the bytes) never travel.
    // Transport: RCCL over xGMI (--rcclId: t4_comm, ncclAllGather + grouped ncclSend / ncclRecv from C++ on the ctx's stream), or
    // files in a directory all ranks see (--gatherDir: the CPU tests; the merge below is the same code).
    if (!useCells) { fprintf(stderr, "trust4-hip: --rcclId / --gatherDir need --barcode (without barcodes the Add pass does not shard).\n"); return EXIT_FAILURE; }
    const std::string tmpRaw = outputPrefix + ".shard" + std::to_string(shardRank) + "_raw.tmp";
    writeSet(tmpRaw);
    std::string rawText;
    readWhole(tmpRaw, rawText);
    unlink(tmpRaw.c_str());
    std::string mainText, rescueText;
    {
      const size_t nMain = assembledReadIdx.size() - (size_t)rescuedCnt;
      formatReads(0, nMain, [&](const std::string &t) { mainText += t; });
      formatReads(nMain, assembledReadIdx.size(), [&](const std::string &t) { rescueText += t; });
    }
    // (1) slots and byte counts of every rank
    std::vector<std::string> heads;
    if (!exchange(std::to_string(cellSlots()) + " " + std::to_string(mainText.size()) + " " + std::to_string(rescueText.size()), true, heads)) { fprintf(stderr, "trust4-hip: the exchange of the shard headers failed\n"); return EXIT_FAILURE; }
    std::vector<long long> slots((size_t)shardCount), mainBytes((size_t)shardCount), rescueBytes((size_t)shardCount);
    for (int r = 0; r < shardCount; ++r) if (sscanf(heads[(size_t)r].c_str(), "%lld %lld %lld", &slots[(size_t)r], &mainBytes[(size_t)r], &rescueBytes[(size_t)r]) != 3) { fprintf(stderr, "trust4-hip: bad shard header from rank %d\n", r); return EXIT_FAILURE; }
    long long base = 0, mainAt = 0, rescueAt = 0, mainAll = 0, slotsAll = 0;
    for (int r = 0; r < shardCount; ++r) { if (r < shardRank) { base += slots[(size_t)r]; mainAt += mainBytes[(size_t)r]; rescueAt += rescueBytes[(size_t)r]; } mainAll += mainBytes[(size_t)r]; slotsAll += slots[(size_t)r]; }
    // (2) `>BARCODE_<id> name` header lines (SeqSet.hpp:10951) of this rank's records: id += base
    std::string renum;
    if (base == 0) renum.swap(rawText);
    else {
      renum.reserve(rawText.size() + rawText.size() / 64);
      const std::string &t = rawText;
      for (size_t i = 0; i < t.size();) {
        size_t e = t.find('\n', i);
        if (e == std::string::npos) e = t.size();
        if (t[i] == '>') {
          size_t sp = t.find(' ', i);
          if (sp == std::string::npos || sp > e) sp = e;
          const size_t us = t.rfind('_', sp - 1);
          renum.append(t, i, us + 1 - i);
          renum += std::to_string(atoll(t.substr(us + 1, sp - us - 1).c_str()) + base);
          renum.append(t, sp, e - sp);
        } else renum.append(t, i, e - i);
        if (e < t.size()) renum.push_back('\n');
        i = e + 1;
      }
    }
    // (3) contig records to rank 0
    std::vector<std::string> raws;
    if (!exchange(renum, false, raws)) { fprintf(stderr, "trust4-hip: the gather of the contig records failed\n"); return EXIT_FAILURE; }
    const std::string readsPath = outputPrefix + "_assembled_reads.fa";
    if (shardRank == 0) {
      for (const char *suffix : {"_raw.out", "_final.out"}) {   // with barcodes _final.out is a second dump of the raw set (main.cpp:2018-2036)
        FILE *fp = fopen((outputPrefix + suffix).c_str(), "wb");
        if (!fp) { fprintf(stderr, "trust4-hip: cannot write %s%s\n", outputPrefix.c_str(), suffix); return EXIT_FAILURE; }
        for (int r = 0; r < shardCount; ++r) fwrite(raws[(size_t)r].data(), 1, raws[(size_t)r].size(), fp);
        fclose(fp);
      }
      FILE *fp = fopen(readsPath.c_str(), "wb");   // created (and emptied) before any rank writes its slice
      if (!fp) { fprintf(stderr, "trust4-hip: cannot write %s\n", readsPath.c_str()); return EXIT_FAILURE; }
      fclose(fp);
    }
    // (4) every rank's slices of _assembled_reads.fa: all main-pass reads by rank, then all rescue-pass reads by rank
    std::vector<std::string> ready;
    if (!exchange("file", true, ready)) { fprintf(stderr, "trust4-hip: the exchange before the read slices failed\n"); return EXIT_FAILURE; }
    {
      const int fd = open(readsPath.c_str(), O_WRONLY);
      if (fd < 0) { fprintf(stderr, "trust4-hip: rank %d cannot open %s\n", shardRank, readsPath.c_str()); return EXIT_FAILURE; }
      auto putAt = [&](const std::string &t, long long at) { size_t done = 0; while (done < t.size()) { const ssize_t w = pwrite(fd, t.data() + done, t.size() - done, (off_t)(at + (long long)done)); if (w <= 0) return false; done += (size_t)w; } return true; };
      const bool ok = putAt(mainText, mainAt) && putAt(rescueText, mainAll + rescueAt);
      close(fd);
      if (!ok) { fprintf(stderr, "trust4-hip: rank %d could not write its reads into %s\n", shardRank, readsPath.c_str()); return EXIT_FAILURE; }
    }
    std::vector<std::string> doneAll;
    if (!exchange("done", true, doneAll)) { fprintf(stderr, "trust4-hip: the last exchange failed\n"); return EXIT_FAILURE; }
    if (shardRank == 0) PrintLog("Gathered %d shards over %s: %lld contig slots.", shardCount, transportNote.c_str(), slotsAll);
    if (const char *sj = getenv("T4_STATS_JSON")) {   // which transport carried the exchange (bench.py reports it: "rccl", "files", or the fallback with its reason)
      FILE *fp = fopen((std::string(sj) + ".transport").c_str(), "w");
      if (fp) { fputs(transportNote.c_str(), fp); fclose(fp); }
    }
    // this rank's files of the exchanges every rank has passed (all but the last) and its status file leave the directory: a later
    // run that is handed the same directory must not take them for its own (launchers hand out fresh directories anyway)
    if (!gatherDir.empty()) for (int no = 0; no + 1 < exchangeNo; ++no) (void)unlink(fileOf(no, shardRank).c_str());
    if (!rcclIdPath.empty()) (void)unlink((rcclIdPath + (lateShard ? ".retry" : "") + ".status.rank" + std::to_string(shardRank)).c_str());
    if (comm) t4_comm_destroy(comm);
    mark("outputs_written");
    writeCellStats();
    destroyCells();
    t4_index_destroy(refSet);
    t4_destroy(ctx);
    return 0;
  }
  // the three files are independent dumps of state that no longer changes: _raw.out and _final.out are written on their own
  // threads while this one writes the reads (stdout output and shards keep the serial order)
  const bool concurrentFiles = !toStdout && shardCount == 1 && threadCnt > 1;
  std::thread rawWriter, finalWriter;
  int rawRc = 0, finalRc = 0; t4_ctx *rawCtx = ctx, *finalCtx = ctx; const char *rawWhat = "", *finalWhat = "";
  if (concurrentFiles) {
    rawWriter = std::thread([&] { rawRc = writeSetRc(outputPrefix + "_raw.out", &rawCtx, &rawWhat); });
    finalWriter = std::thread([&] { finalRc = writeSetRc(outputPrefix + "_final.out", &finalCtx, &finalWhat); });
  } else writeSetOrStdout(outputPrefix + "_raw.out");
  size_t nMainAssembled = assembledReadIdx.size();
  if (shardCount > 1) nMainAssembled -= (size_t)rescuedCnt;
  {
    auto writeReads = [&](const std::string &path, size_t lo, size_t hi) {
      FILE *fp = fopen(path.c_str(), "w");
      if (!fp) { fprintf(stderr, "trust4-hip: cannot write %s\n", path.c_str()); exit(EXIT_FAILURE); }
      bool ok = true;
      formatReads(lo, hi, [&](const std::string &t) { if (!t.empty() && fwrite(t.data(), 1, t.size(), fp) != t.size()) ok = false; });
      if (fclose(fp) != 0 || !ok) { fprintf(stderr, "trust4-hip: writing %s failed\n", path.c_str()); exit(EXIT_FAILURE); }
    };
    writeReads(outputPrefix + "_assembled_reads.fa", 0, nMainAssembled);
    // a shard keeps the rescue-pass reads apart: the merged file lists them after every shard's main pass
    if (shardCount > 1 && nMainAssembled < assembledReadIdx.size()) writeReads(outputPrefix + "_assembled_reads_rescue.fa", nMainAssembled, assembledReadIdx.size());
  }
  if (shardCount > 1) {   // contig ids above are local to the shard; stage1_dist.py shifts them by the slots of the earlier shards
    if (nMainAssembled == assembledReadIdx.size()) { FILE *fp = fopen((outputPrefix + "_assembled_reads_rescue.fa").c_str(), "w"); if (fp) fclose(fp); }
    FILE *fp = fopen((outputPrefix + "_shard.meta").c_str(), "w");
    fprintf(fp, "shard %d %d\ncontig_slots %d\nreads %d\n", shardRank, shardCount, cellSlots(), readCnt);
    fclose(fp);
  } else {
    if (!skipMateExtension && hasMate && !hasBarcode)   // only reachable under --allowRawFinal (checked with the options)
      PrintLog("NOTE: --allowRawFinal: _final.out is the raw assembly (what the reference writes under --skipMateExtension), NOT its mate-pair extension.");
    if (!concurrentFiles) writeSetOrStdout(outputPrefix + "_final.out");
  }
  if (concurrentFiles) {
    rawWriter.join(); finalWriter.join();
    if (rawRc) die(rawCtx, rawWhat, rawRc);
    if (finalRc) die(finalCtx, finalWhat, finalRc);
  }
  if (useCells) {
    mark("outputs_written");
    writeCellStats();
    leave(0);
    destroyCells();
    t4_index_destroy(refSet);
    t4_destroy(ctx);
    return 0;
  }
  int64_t q = 0, rf = 0, wh = 0;
  t4_assembler_counters(seqSet, &q, &rf, &wh);
  double sr = 0, sq = 0;
  t4_assembler_timers(seqSet, &sr, &sq);
  int64_t lc[30] = {0};
  t4_assembler_live_counters(seqSet, lc, 30);
  mark("outputs_written");
  if (const char *sj = getenv("T4_STATS_JSON")) {
    FILE *fp = fopen(sj, "w");
    if (fp) {
      fprintf(fp, "{\"reads\": %d, \"threads\": %d, \"phases_s\": {", readCnt, threadCnt);
      for (size_t i = 0; i < phaseMarks.size(); ++i) fprintf(fp, "%s\"%s\": %.4f", i ? ", " : "", phaseMarks[i].first.c_str(), phaseMarks[i].second);
      fprintf(fp, "}, \"rough_annotation\": {\"reads\": %lld, \"hits\": %lld, \"kernel_ms\": %.3f}, ", annotReads, annotHits, annotKernelMs);
      fprintf(fp, "\"add_query\": {\"rounds\": %lld, \"reads_queried\": %lld, \"reads_served\": %lld, \"kernel_ms\": %.3f, \"hits\": %lld, \"records\": %lld, "
                  "\"global_tier_launches\": %lld, \"global_tier_reads\": %lld, \"deltas\": %lld, \"delta_bytes\": %lld, \"invalidations\": %lld, \"host_wait_for_queries_s\": %.3f, "
                  "\"wide\": {\"reads\": %lld, \"partitions\": %lld, \"calls_repeated\": %lld, \"dependency_records\": %lld}, "
                  "\"long_lists\": {\"restricted_merged\": %lld, \"fell_whole\": %lld}}, ",
              (long long)lc[0], (long long)lc[1], (long long)wh, lc[21] / 1e3, (long long)lc[22], (long long)lc[20], (long long)lc[18], (long long)lc[19], (long long)lc[2],
              (long long)lc[3], (long long)lc[4], lc[15] / 1e6, (long long)lc[23], (long long)lc[24], (long long)lc[25], (long long)lc[26], (long long)lc[28], (long long)lc[29]);
      double cs[10] = {0};
      t4_assembler_chain_stats(seqSet, cs, 10);
      fprintf(fp, "\"chain\": {\"rounds\": %.0f, \"restricted_only_rounds\": %.0f, \"round_kernel_ms_p05\": %.4f, \"round_kernel_ms_p50\": %.4f, \"round_wall_ms_p05\": %.4f, \"round_wall_ms_p50\": %.4f, "
                  "\"whole_queries\": %.0f, \"restricted_queries\": %.0f, \"candidate_records\": %.0f, \"restricted_merged_by_replay\": %.0f}, ",
              cs[0], cs[1], cs[2], cs[3], cs[4], cs[5], cs[6], cs[7], cs[8], cs[9]);
      fprintf(fp, "\"text_counts\": {\"on\": %d, \"batches\": %lld, \"kept\": %lld}, ", textCounts.on ? 1 : 0, textCounts.batches, textCounts.batchesKept);
      fprintf(fp, "\"contigs\": %d, \"assembled_reads\": %d}\n", t4_assembler_size(seqSet), (int)assembledReadIdx.size());
      fclose(fp);
    }
  }
  if (getenv("T4_TIMING")) PrintLog("timing: AddRead query path: %lld calls, %lld reads, global-scratch tier %lld launches for %lld reads, %lld result records", (long long)lc[16], (long long)lc[17], (long long)lc[18], (long long)lc[19], (long long)lc[20]);
  PrintLog("Finish assembly. (GPU query rounds %lld with %lld reads in %.2f s; %lld image deltas, %.1f MB, in %.2f s; reads served from the window %lld; "
           "window entries invalidated %lld: key %lld, list>=100 %lld, region %lld, shift %lld, contig %lld, tolerance %lld; tolerated index changes %lld; "
           "dependency sets %.2f s, event examination %.2f s)",
           (long long)lc[0], (long long)lc[1], lc[15] / 1e6, (long long)lc[2], lc[3] / 1e6, lc[12] / 1e6, (long long)wh, (long long)lc[4], (long long)lc[5], (long long)lc[6],
           (long long)lc[7], (long long)lc[8], (long long)lc[9], (long long)lc[10], (long long)lc[11], lc[13] / 1e6, lc[14] / 1e6);
  (void)q; (void)rf; (void)sr; (void)sq;
  leave(0);
  t4_assembler_destroy(seqSet);
  t4_index_destroy(refSet);
  t4_destroy(ctx);
  return 0;
}
