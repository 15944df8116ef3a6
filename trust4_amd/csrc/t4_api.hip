// trust4_amd/csrc/t4_api.hip -- C ABI of libt4hip.so (include/trust4_hip.h): host side of the engine.
// Sequence-set construction follows SeqSet::InputRefFa / InputNovelRead and
// KmerIndex::BuildIndexFromRead (SeqSet.hpp:2673-2865, 3028-3073; KmerIndex.hpp:118-141); the k-mer
// index is flattened into CSR postings + a direct-addressed (k <= 12) or open-addressing table that
// stays resident in HBM/L2. Queries run as: bin reads by hit count -> one persistent-grid launch per
// capacity tier (reads that outgrow a tier are re-queued on the next one).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#ifdef __HIPCC__
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is bound by dlopen in t4_comm_init
#include <type_traits>
#include <unistd.h>
#endif
#include "../../include/trust4_hip.h"
#include "t4_kernels.h"
#include "t4_text.h"
#include "t4_internal.h"

static_assert(sizeof(t4_overlap) == sizeof(T4OverlapOut), "overlap layout");
static_assert(sizeof(t4_hit) == sizeof(T4HitOut), "hit layout");
static_assert(sizeof(t4k::OvRec) == 40, "OvRec layout");
static_assert(sizeof(T4IndexView) % 16 == 0, "view stride");

namespace {

// per capacity tier: LDS hit capacity, threads cooperating on one read, resident workgroups per CU
const int TIER_CAP[T4_NTIER - 1] = {1024, 2048, 3072, 4096, 8192};
// Reads in flight per CU are what counts (most phases of a read are latency bound): tier 0 runs 8 groups of 2 waves in
// 8 x 20 KB of LDS, tier 1 4 groups of 4 waves in 4 x 39 KB, both at 128 VGPRs (4 waves / SIMD); the 3072-hit tier exists
// because 3 of its groups fit a CU where only 2 of the 4096-hit tier do. 512/1024 threads per read in the upper tiers
// measured slower (barriers).
const int TIER_THREADS[T4_NTIER] = {128, 256, 256, 256, 512, 512};   // the 8192-hit tier has one group per CU (LDS): eight waves of it
const int TIER_BLOCKS_PER_CU[T4_NTIER] = {8, 4, 3, 2, 1, 2};
// global-scratch tier: hits and overlaps of one read pass (SURVEY 6 measured 50 036 hits for one AssignRead query at k = 17 and
// 100 k pairs; a read of a gene segment that thousands of contigs share meets every one of them)
const int G_CAP = 262144, G_MAXOV = 16384;
constexpr int G_THREADS = 512;

struct HostSeq {
  std::string name, cons;
  std::vector<int32_t> pw;  // 4 per base, novel only
  int barcode;
  bool isRef;
};

}  // namespace

struct t4_ctx;
static int fail(t4_ctx *c, int code, const char *fmt, ...);
#define HIPCHK(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return fail((ctx), T4_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// ---- owners of device memory, pinned memory, streams and events ---------------------------------------------------
// Every handle keeps its GPU resources in these: move-only, freed by the destructor, null after a failed allocation. Members are
// destroyed in reverse order of declaration, so a handle declares its streams and events before the buffers they work on.
// What a kernel reads (T4Wide, T4KmerTable, the views, the blobs) stays plain structs of raw pointers, filled from the owners.
// Device memory: a call's own (freed on every way out of the scope) or a handle's. hipFree waits for the work that still uses it.
template <class T> struct DevBuf {
  T *p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf &&o) : p(o.p) { o.p = nullptr; }   // (move only)
  DevBuf &operator=(DevBuf &&o) { swap(o); return *this; }   // (what was here goes with o)
  ~DevBuf() { free(); }
  void swap(DevBuf &o) { std::swap(p, o.p); }
  void free() { if (p) (void)hipFree(p); p = nullptr; }
  int alloc(t4_ctx *c, size_t count) {   // frees first: a growth that fails leaves nothing behind
    free();
    HIPCHK(c, hipMalloc(&p, sizeof(T) * (count ? count : 1)));
    return T4_OK;
  }
  // to `want` elements keeping the first `keep` (stream-ordered copy; the old block is freed once the copy is done)
  int growKeep(t4_ctx *c, int64_t keep, int64_t want);
  operator T *() const { return p; }
};
// Pinned host memory; with hipHostMallocMapped also its address on the device, asked for once, here.
template <class T> struct PinnedBuf {
  T *p = nullptr, *dev = nullptr;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) : p(o.p), dev(o.dev) { o.p = o.dev = nullptr; }
  ~PinnedBuf() { free(); }
  void swap(PinnedBuf &o) { std::swap(p, o.p); std::swap(dev, o.dev); }
  void free() { if (p) (void)hipHostFree(p); p = dev = nullptr; }
  int alloc(t4_ctx *c, size_t count, unsigned flags) {
    free();
    HIPCHK(c, hipHostMalloc(&p, sizeof(T) * (count ? count : 1), flags));
    if (flags & hipHostMallocMapped) {
      const hipError_t e = hipHostGetDevicePointer((void **)&dev, p, 0);
      if (e != hipSuccess) { free(); return fail(c, T4_ERR_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e)); }
    }
    return T4_OK;
  }
  operator T *() const { return p; }
};
// One stream / one event: made by create() (where the code makes them lazily, that is a no-op from the second time on).
struct Stream {
  hipStream_t s = 0;
  Stream() = default;
  Stream(const Stream &) = delete;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create() { return s ? hipSuccess : hipStreamCreate(&s); }
  operator hipStream_t() const { return s; }
};
struct Event {
  hipEvent_t e = 0;
  Event() = default;
  Event(const Event &) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return e ? hipSuccess : hipEventCreate(&e); }
  operator hipEvent_t() const { return e; }
};
// The device pools of the wide query (t4_wide.h) with their elements per read slot / per partition: what ensureWide allocates,
// what wideHalf steps over and what WidePools frees.
template <class F> void widePoolsPerRead(T4Wide &w, F f) {
  f(w.seed, T4_WIDE_SEEDS); f(w.bounds, T4_WIDE_MAXP + 1); f(w.uniqPref, w.pcap + 1); f(w.sortTmp, 2 * (size_t)w.pcap); f(w.requeue, 1);
}
template <class F> void widePoolsPerPart(T4Wide &w, F f) {
  f(w.pCnt, 1); f(w.pRead, 1); f(w.pKeys, w.pcap); f(w.gSize, w.pcap); f(w.gInfo, w.pcap); f(w.gCount, 4); f(w.gOff, 2);
  f(w.pRec, (size_t)w.maxOvPart * 10); f(w.pRecCnt, 1); f(w.mKeys, w.maxOvPart); f(w.mOrd, w.maxOvPart);
}
// T4Wide (device pointers + capacities; a copy travels in every call's input blob) as the ctx holds it: the owner of its pools.
struct WidePools : T4Wide {
  bool init = false;
  PinnedBuf<T4Grp> grpHost;        // T4Wide::grpPool is its device address
  PinnedBuf<unsigned> headHost;    // T4Wide::headBits is its device address
  WidePools() { memset(static_cast<T4Wide *>(this), 0, sizeof(T4Wide)); }
  WidePools(const WidePools &) = delete;
  ~WidePools() {
    auto drop = [](auto *&p, size_t) { if (p) (void)hipFree(p); p = nullptr; };
    widePoolsPerRead(*this, drop); widePoolsPerPart(*this, drop);
  }
  template <class T> static int alloc(t4_ctx *c, T *&p, size_t count) {   // one pool: freed first, null on failure
    if (p) (void)hipFree(p);
    p = nullptr;
    HIPCHK(c, hipMalloc(&p, sizeof(T) * (count ? count : 1)));
    return T4_OK;
  }
};

// A field of one of the call's two blobs: `count` elements of T, declared once in AqInput / AqHeader. The input blob is packed in
// pinned staging memory and copied to the device by aqPrologueKernel; the header blob is written on the device and copied into
// pinned host memory by aqEpilogueKernel.
template <class T> struct AqField {
  size_t off = 0;
  bool header = false;
  T *stage(const t4_ctx *c) const;        // input blob: the host's staging copy
  T *dev(const t4_ctx *c) const;          // either blob: the device copy
  const T *host(const t4_ctx *c) const;   // header blob: the pinned copy on the host
};
struct AqBlob {   // fields are appended in the order of the blob, each at the next multiple of 8 bytes
  bool header = false;
  size_t bytes = 0;
  template <class T> void add(AqField<T> &f, size_t count) { f.off = bytes; f.header = header; bytes = (bytes + sizeof(T) * count + 7) & ~(size_t)7; }
};
struct AqInput : AqBlob {
  AqField<unsigned> pk, nm;
  AqField<int> len, barcode, strand, list /* the work lists: first launch, then second stream */, viewOf;
  AqField<double> factor;
  AqField<int> onlySeq, forceMin;
  AqField<int> arm; AqField<unsigned> head;   // armed restricted re-queries (hasArm): T4CandArgs::rorArm, rorHead; empty otherwise
  AqField<T4CandArgs> cs;
  AqField<T4Wide> wide[2];   // the two halves of the wide query (wideHalf)
};
struct AqHeader : AqBlob {
  AqField<int> counts, status, next, next2, outBase, ticks, stable, aux, n4, candBase, candCnt, stats8;
  AqField<int> rorInfo;      // hasArm: T4CandArgs::rorInfo; empty otherwise
  AqField<T4AqTail> tail;
  struct { AqField<int> ctl; AqField<T4WidePlan> plan; AqField<int> stat; } wide[2];   // per half: T4Wide::ctl, plan, stat (nWideSlots read slots)
};

// The call is split in two so that a caller can keep the host busy while the kernels run (t4_assembler commits reads whose cached
// queries still stand): aqBegin packs the input and enqueues copies + kernels + the header copy on the ctx's stream; aqEnd waits
// for them, runs whatever overflow launch is still needed (rare paths, synchronous) and hands out the result. One call in flight
// per ctx. tierHint must stay alive until aqEnd.
struct AqCall {
  bool active = false;
  T4IndexView base; const T4IndexView *views = nullptr; bool hasViewOf = false, smallFirst = false, lean = false;
  int n = 0, skipRepeats = 0, wpk = 0, wnm = 0, attempt = 0, nFirst = 0, nDirect = 0, threads = 512;
  unsigned char *tierHint = nullptr;
  std::vector<unsigned char> allGlobal;
  AqInput in; AqHeader hdr;
  bool hasOnly = false, hasForce = false, wantCands = false;
  bool hasArm = false;   // restricted re-queries of reads with long lists, armed by t4_add_query_arm_long_lists (T4CandArgs::rorArm)
  bool keepExtAux = false;   // t4_assign_wide: one word per pool record beside the public records (T4CandArgs::extAux)
  bool extendLater = false, wide = false, onlyRestricted = false;
  bool sweep2Done = false;     // the second sweep of the wide kernels (first passes of skipRepeats queries that found nothing) has been looked at
  int nWideSlots = 0;          // read slots per half of the wide query's header arrays (2 n for a skipRepeats call: a read may take one per sweep)
  bool lazyDone = false, lazyStage = false;   // the wide pipeline behind the query kernel is launched only once the kernel is known to have deferred a read (aqEnd)
  int wideSafety = 32;   // of sixteenths: partitions are planned for half of their capacity
  T4BatchView bv; T4QueryArgs qa; T4Work wk;
  std::chrono::steady_clock::time_point tf0;
};

struct t4_ctx {
  int device = 0, cus = 0;
  // (streams and events first: the buffers below are freed before these are destroyed)
  Stream stream;
  Stream stream2;   // AddRead queries: reads known to need the global-scratch tier run beside the LDS tier; made with evIn, evG by the first call that has such reads
  Event evIn, evG;
  Event ev[4];
  std::string err;
  t4_stats stats;
  // scratch
  int maxGrid = 0;
  DevBuf<int> dpRows;
  DevBuf<unsigned char> dpDir;
  DevBuf<unsigned long long> gKeys;
  DevBuf<unsigned> gPairs;
  DevBuf<int> gOv, gFin;
  DevBuf<unsigned short> gOrd;
  int gGrid = 0;
  DevBuf<unsigned long long> hitsKeys;
  int hitsGrid = 0;
  // per-call buffers (grown on demand)
  DevBuf<int> lists, listCounts, status, counts;
  long long listCap = 0;
  DevBuf<unsigned long long> hitCounter;
  DevBuf<T4OverlapOut> result;
  size_t resultCap = 0, resultBytes = 0;
  // lean path of t4_add_query (small batches, one launch, one round trip)
  int aqCap = 0, aqWpk = 0, aqWnm = 0, aqMax = 0;
  DevBuf<unsigned char> aqIn, aqOut;      // device blobs
  PinnedBuf<unsigned char> aqInHost, aqOutHost;   // pinned staging, mapped: aqPrologueKernel reads the one, aqEpilogueKernel writes the other
  PinnedBuf<unsigned> aqFlag;   // pinned word the epilogue of a call leaves the call's sequence number in: what the host waits for
  DevBuf<unsigned> aqDoneCtr;   // device: blocks of a running epilogue that have written their share
  unsigned aqSeq = 0;
  size_t aqInBytes = 0, aqOutBytes = 0;
  PinnedBuf<unsigned char> aqPool;   // result records of t4_add_query*: pinned host memory the kernels write
  int aqPoolCap = 0;
  PinnedBuf<unsigned char> candPool;   // candidate store of t4_add_query_pool_begin2 (pinned host memory the kernels write)
  int candCap = 0, candGrows = 0;
  int64_t candRecords = 0;
  DevBuf<T4OverlapOut> aqRecDev;   // device copy of the overlap records + the read of each, for the extension launch
  DevBuf<int> aqRecRead;
  int aqRecCap = 0;
  DevBuf<int> aqExtAux;   // T4CandArgs::extAux of the calls t4_assign_wide makes: one word per record of the result pool
  int aqExtAuxCap = 0;
  int64_t assignWide[2] = {0, 0};   // last t4_assign_wide call: reads answered by the single-workgroup tiers, reads answered by the wide route
  int64_t aqCalls = 0, aqReads = 0, aqGlobalLaunches = 0, aqGlobalReads = 0, aqRecords = 0;
  double aqSecPack = 0, aqSecFirst = 0, aqSecGlobal = 0;
  double aqSecLaunch[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // host seconds inside aqLaunch: preparation, prologue, second stream, query kernel, wide + extension, events, epilogue
  int aqPoolGrows = 0;
  const int32_t *aqLastStable = nullptr;   // per-read flags of the last AddRead query call: group statistics that index edits of small groups cannot move
  const int32_t *aqLastTicks = nullptr; int aqLastN = 0;   // per-read wall-clock ticks (10 ns) of the last AddRead query call (in the pinned header blob)
  double aqLastMs = 0;
  AqCall aq;
  uint64_t textScans = 0;   // t4_text_scan calls of the ctx's handles so far: every scan has a number of its own (t4_text::scanId)
  uint64_t syncEpoch = 1;   // bumped whenever the ctx's stream has been waited for: work queued before that is done (t4_index_apply_delta's staging buffer)
  // testing aids of the AddRead query path, read from the environment once per ctx (a query round is a few hundred microseconds; a
  // dozen getenv calls in it are not nothing)
  struct AqEnv {
    bool forceGlobal;
    int capLimit, extendDefer, poolCap, candCap, wideMinHits;
    AqEnv() {
      auto num = [](const char *n, int d) { const char *e = getenv(n); return e ? atoi(e) : d; };
      forceGlobal = getenv("T4_AQ_FORCE_GLOBAL") != nullptr;
      capLimit = num("T4_AQ_CAP_LIMIT", 0); poolCap = num("T4_AQ_POOL_CAP", 0); candCap = num("T4_AQ_CAND_CAP", 1 << 18);
      // (64 until round 5: with light rounds extendKernel runs behind the whole-query rounds anyway, and a read's 17th overlap is better
      // off there -- profiles/r05e, r05f)
      extendDefer = num("T4_AQ_EXTEND_DEFER", 16);
      wideMinHits = num("T4_WIDE_MIN_HITS", 3072);   // (round 6: 3 072 -- kernels of C2 23.9 -> 23.6 s, 2 % fewer rounds, profiles/r06g; 4 096 in round 5:)   // (8192, the LDS tier's capacity, until round 5: fresh heavy reads now start on the wide pipeline beside the query kernel, so the wide query pays from half of it on -- C2 67.5 -> 61.0 s, profiles/r05e_c2_w4k, r05f)
    }
  } aqEnv;
  // the wide query (t4_wide.h): pools of the deferred reads of one call, grown on demand
  WidePools wide;            // device pointers + capacities (a copy travels in every call's input blob)
  std::vector<int32_t> armWords;          // t4_add_query_arm_long_lists: T4CandArgs::rorArm of the next call with restricted re-queries (2 per read)
  std::vector<uint32_t> armHead;          // ... and the head bitmaps its second words point into
  int64_t wideReads = 0, wideParts = 0, wideRetries = 0, wideGroups = 0;
  int64_t aqDeferredReads = 0;   // reads whose ExtendOverlap calls the query kernel left to extendKernel (T4QueryArgs::extendLater)
  int64_t wideCalls = 0, wideCallsDeferred = 0, wideCallsDirect = 0;   // calls with the wide query on; those whose query kernel deferred a read; those with reads on the second stream
  int wideSafetyKeep = 32, wideCallsSinceRepeat = 0;   // partition load factor that recent calls needed (of sixteenths: 32 = partitions planned half full); decays back when nothing overflows
  int64_t wideFlagCounts[6] = {0, 0, 0, 0, 0, 0};     // calls repeated because: reads, partitions, keys of a partition, overlaps of a partition, dependency records, other
  int wideRecentParts = 0;   // the largest partition counts of the last calls, decayed: sizes the (persistent) grids of the next call's second-stream wide kernels
  double aqKernelMs = 0;    // HIP-event time of the query kernels of all AddRead query calls (per call: first launch .. last kernel)
  int64_t aqHits = 0;       // _hit records their seed stages emitted (H of SURVEY 8d)
};
template <class T> T *AqField<T>::stage(const t4_ctx *c) const { return (T *)(c->aqInHost.p + off); }
template <class T> T *AqField<T>::dev(const t4_ctx *c) const { return (T *)((header ? c->aqOut.p : c->aqIn.p) + off); }
template <class T> const T *AqField<T>::host(const t4_ctx *c) const { return (const T *)(c->aqOutHost.p + off); }

struct t4_index {
  t4_ctx *ctx;
  int k, considerBarcode;
  int hitLenRequired = 31, radius = 10;
  double novelSim = 0.9, refSim = 0.75, repeatSim = 0.95;
  int nomatchGapLimit;
  std::vector<HostSeq> seqs;
  std::unordered_map<std::string, int> dedup;
  bool committed = false;
  // device image
  Event stEvent;   // (first: destroyed after the buffers)
  DevBuf<uint2> dTable;
  DevBuf<T4HashEnt> dHtab;
  DevBuf<int2> dPost;
  DevBuf<T4SeqInfo> dSeqs;
  DevBuf<char> dCons;
  DevBuf<T4PW> dPw;
  T4IndexView view;
  // live set (t4_index_apply_delta): capacities of the four arrays, staging of one delta
  bool live = false;
  DevBuf<T4HashEntC> dCtab;
  int64_t capTable = 0, capPost = 0, capBase = 0;
  int capSeq = 0, liveNseq = 0;
  PinnedBuf<unsigned char> stHost;   // (mapped: a small delta is read by the kernel straight out of it)
  DevBuf<unsigned char> stDev;
  size_t stCap = 0;
  bool stPending = false;
  uint64_t stEpoch = 0;      // the ctx's syncEpoch when the staging buffer was last handed to a copy
};

struct t4_batch {
  t4_ctx *ctx;
  long long n = 0;
  int wpk = 0, wnm = 0, maxLen = 0;
  DevBuf<unsigned> dPk, dNm;
  DevBuf<int> dLen, dBarcode;
  int minBarcode = -1, maxBarcode = -1;   // of dBarcode, from the host array it was uploaded from (per-barcode k-mer counts: kmerBarcodesFit)
  DevBuf<unsigned char> dLow;   // low-complexity bytes (batches of t4_text_batch; null otherwise: no read counts as low)
  DevBuf<char> dQual;           // batches of t4_text_pairs_batch made with qualities: the rows' quality bytes, qualBytes of them ...
  DevBuf<long long> dQoff;      // ... and where each row's begin (n + 1 offsets); null otherwise
  long long qualBytes = 0;
  T4BatchView view;
};

// FASTQ text on the device (t4_text.h): everything one piece needs, allocated once for pieces of up to `cap` bytes.
struct t4_text {
  t4_ctx *ctx = nullptr;
  int64_t cap = 0;
  PinnedBuf<char> stage;                      // the piece on its way to the device
  PinnedBuf<unsigned long long> infoHost;     // T4_TEXT_INFO_WORDS words to and from dInfo
  DevBuf<char> dText;                         // whole tiles
  DevBuf<unsigned> dTileCnt, dLineStart;      // per tile; per line + 1
  DevBuf<int> dLen;                           // per record of the piece (at most cap / 4) ...
  DevBuf<unsigned> dRecStart;
  DevBuf<unsigned char> dLow;
  DevBuf<unsigned long long> dInfo;
  // t4_text_process_pairs with this handle as `reads`: made by the first call, reused
  DevBuf<int4> dPairMeta;                     // per record of the piece
  DevBuf<unsigned char> dPairSkip;
  DevBuf<char> dPairR, dPairQ;                // changed reads and their qualities, pairCap bytes each
  DevBuf<unsigned long long> dPairNeed;       // bytes the changed reads take
  PinnedBuf<unsigned long long> pairNeedHost;
  int64_t pairCap = 0;
  // the last t4_text_process_pairs call with this handle as `reads`: whether it succeeded, what it covered and which scans it looked at
  bool pairOk = false;
  const t4_text *pairMates = nullptr;
  int64_t pairFirst[2] = {0, 0}, pairN = 0;
  uint64_t pairScan[2] = {0, 0};
  // t4_text_pairs_batch with this handle as `reads`: made by the first call, reused
  DevBuf<uint2> dRowAt;                       // per record of the piece: rows and bases ahead of the pair in its workgroup
  DevBuf<unsigned long long> dRowBlock;       // per workgroup of T4_TEXT_THREADS pairs: rows, then bases
  DevBuf<unsigned long long> dRowInfo;        // T4_PAIRROWS_WORDS words
  PinnedBuf<unsigned long long> rowInfoHost;
  // the piece last scanned
  uint64_t scanId = 0;                        // which scan of the ctx (t4_ctx::textScans) it was: 0 none
  int status = -1;                            // -1: none
  int64_t nbytes = 0, lines = 0, nrec = 0, recBytes = 0, badRec = -1;
  int longest = 0;
};

static int fail(t4_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}
template <class T> int DevBuf<T>::growKeep(t4_ctx *c, int64_t keep, int64_t want) {
  DevBuf<T> grown;
  HIPCHK(c, hipMalloc(&grown.p, sizeof(T) * (size_t)(want > 0 ? want : 1)));
  if (p && keep > 0) HIPCHK(c, hipMemcpyAsync(grown.p, p, sizeof(T) * (size_t)keep, hipMemcpyDeviceToDevice, c->stream));
  if (p) HIPCHK(c, hipStreamSynchronize(c->stream));
  swap(grown);   // (the old block goes with `grown`)
  return T4_OK;
}
namespace {

// A launch whose arguments are turned into the kernel's parameter types first (a DevBuf into its pointer: the buffer itself is not copied).
template <class T> struct AsIs { typedef T type; };
template <class... P> void launch(void (*kernel)(P...), int grid, int block, hipStream_t stream, typename AsIs<P>::type... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, args...);
}

// SeqSet::GetChainType / GetGeneType (SeqSet.hpp:5132-5155, 5076-5100)
int chainType(const char *n) {
  if (n[0] == 'I') { if (n[2] == 'H') return 0; if (n[2] == 'K') return 1; if (n[2] == 'L') return 2; }
  else if (n[0] == 'T') { if (n[2] == 'A') return 3; if (n[2] == 'B') return 4; if (n[2] == 'G') return 5; if (n[2] == 'D') return 6; }
  return 8;
}
int geneType(const char *n) {
  if (n[0] == 'N' && n[1] == 'o') return -1;
  switch (n[3]) {
    case 'V': return 0;
    case 'D': return (n[4] >= '0' && n[4] <= '9') ? 1 : 3;
    case 'J': return 2;
    case 'L': if (chainType(n) == 2) return -1; return 3;
    default: return 3;
  }
}
inline int nucNum(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// gap-DP scratch for `threads` resident threads (fallback path of bands wider than a wavefront)
int ensureScratch(t4_ctx *c, int threads) {
  if (threads <= c->maxGrid) return T4_OK;
  c->maxGrid = 0;   // alloc frees first: a growth that fails leaves no capacity behind, and the next call starts over
  int r;
  if ((r = c->dpRows.alloc(c, (size_t)(threads / 64 + 1) * 6 * T4_ROWW * 64))) return r;
  if ((r = c->dpDir.alloc(c, (size_t)threads * T4_DIR_BYTES))) return r;
  c->maxGrid = threads;
  return T4_OK;
}
int ensureGlobalTier(t4_ctx *c, int grid) {
  if (grid <= c->gGrid) return T4_OK;
  { int g = c->gGrid > 0 ? c->gGrid : 32; while (g < grid) g *= 2; grid = g; }   // 5.4 MB per block: grow rarely
  c->gGrid = 0;
  int r;
  if ((r = c->gKeys.alloc(c, (size_t)grid * G_CAP))) return r;
  if ((r = c->gPairs.alloc(c, (size_t)grid * G_CAP * 2))) return r;   // pairs + cand, contiguous per block
  if ((r = c->gOv.alloc(c, (size_t)grid * G_MAXOV * 10))) return r;
  if ((r = c->gFin.alloc(c, (size_t)grid * G_MAXOV * 10))) return r;
  if ((r = c->gOrd.alloc(c, (size_t)grid * G_MAXOV))) return r;
  c->gGrid = grid;
  return T4_OK;
}
int ensurePerCall(t4_ctx *c, long long n) {
  if (n <= c->listCap) return T4_OK;
  c->listCap = 0;
  int r;
  if ((r = c->lists.alloc(c, (size_t)n * T4_NTIER))) return r;
  if ((r = c->status.alloc(c, (size_t)n))) return r;
  if ((r = c->counts.alloc(c, (size_t)n))) return r;
  c->listCap = n;
  return T4_OK;
}


// pools of the wide query (t4_wide.h): room for `reads` deferred reads, `parts` partitions of `pcap` keys and `groups` dependency
// records per call; existing contents are never needed across calls, so growing reallocates
int wideEnv(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
size_t wideHeadWords(const T4Wide &w) { return (size_t)(w.pcap + 31) / 32; }   // of T4Wide::headBits (pinned), per read slot
int ensureWide(t4_ctx *c, int reads, int parts, int groups) {
  WidePools &w = c->wide;
  if (!w.init) {
    w.pcap = wideEnv("T4_WIDE_PCAP", 8192);   // testing aid: small partitions, so that small inputs spread over several
    if (w.pcap < 64) w.pcap = 64;
    if (w.pcap > 8192) w.pcap = 8192;
    w.maxOvPart = 1 << T4_WIDE_OVBITS;
    w.maxPartPerRead = T4_WIDE_MAXP;
    w.init = true;
  }
  int r;
  if (reads > w.maxReads) {
    int n = w.maxReads > 0 ? w.maxReads : 64;
    while (n < reads) n *= 2;
    w.maxReads = 0;
    r = T4_OK;
    widePoolsPerRead(w, [&](auto *&p, size_t per) { if (!r) r = WidePools::alloc(c, p, 2 * (size_t)n * per); });   // (two of everything: wideHalf)
    if (r) return r;
    w.headBits = nullptr;
    if ((r = w.headHost.alloc(c, 2 * (size_t)n * wideHeadWords(w), hipHostMallocMapped))) return r;
    w.headBits = w.headHost.dev;
    w.maxReads = n;
  }
  if (parts > w.maxPart) {
    int n = w.maxPart > 0 ? w.maxPart : wideEnv("T4_WIDE_PARTS", 1024);
    while (n < parts) n *= 2;
    w.maxPart = 0;
    r = T4_OK;
    widePoolsPerPart(w, [&](auto *&p, size_t per) { if (!r) r = WidePools::alloc(c, p, 2 * (size_t)n * per); });
    if (r) return r;
    w.maxPart = n;
  }
  if (groups > w.grpCap) {
    int n = w.grpCap > 0 ? w.grpCap : wideEnv("T4_WIDE_GROUPS", 1 << 20);
    while (n < groups) n *= 2;
    w.grpPool = nullptr; w.grpCap = 0;
    if ((r = w.grpHost.alloc(c, 2 * (size_t)n, hipHostMallocMapped))) return r;
    w.grpPool = w.grpHost.dev;
    w.grpCap = n;
  }
  return T4_OK;
}
// The pools hold two pipelines' worth: half 0 serves the reads the round's query kernel defers, half 1 the reads that were known to
// be heavy and started on the second stream (wideSeedKernel).
T4Wide wideHalf(const t4_ctx *c, int half) {
  T4Wide w = c->wide;
  if (!half) return w;
  const size_t R = (size_t)w.maxReads, P = (size_t)w.maxPart;
  widePoolsPerRead(w, [&](auto *&p, size_t per) { p += R * per; });
  widePoolsPerPart(w, [&](auto *&p, size_t per) { p += P * per; });
  w.headBits += R * wideHeadWords(w);
  w.grpPool += w.grpCap;
  return w;
}

}  // namespace

extern "C" {

int t4_init(int device_ordinal, t4_ctx **out) {
  if (!out) return T4_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_ordinal < 0 || device_ordinal >= ndev) return T4_ERR_HIP;
  if (hipSetDevice(device_ordinal) != hipSuccess) return T4_ERR_HIP;
  std::unique_ptr<t4_ctx> c(new t4_ctx());   // (every failure below frees what was made so far: the ctx's members own it)
  c->device = device_ordinal;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return T4_ERR_HIP;
  c->cus = prop.multiProcessorCount;
  if (c->stream.create() != hipSuccess) return T4_ERR_HIP;
  for (Event &e : c->ev) if (e.create() != hipSuccess) return T4_ERR_HIP;
  memset(&c->stats, 0, sizeof c->stats);
  if (c->listCounts.alloc(c.get(), 16) || c->hitCounter.alloc(c.get(), 1)) return T4_ERR_HIP;
  if (c->aqFlag.alloc(c.get(), 16, hipHostMallocMapped) || c->aqDoneCtr.alloc(c.get(), 1) || hipMemset(c->aqDoneCtr, 0, sizeof(unsigned)) != hipSuccess) return T4_ERR_HIP;
  *c->aqFlag.p = 0;
  *out = c.release();
  return T4_OK;
}

void t4_destroy(t4_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
#ifdef T4_PHASE_TIMING
  if (getenv("T4_PHASE_DUMP")) {   // development aid: cycles per kernel phase over the life of the ctx
    unsigned long long ph[T4_NPHASE];
    if (hipMemcpyFromSymbol(ph, HIP_SYMBOL(t4k::g_phaseCycles), sizeof(ph)) == hipSuccess) {
      static const char *names[32] = {"other", "seed:lookup", "expand", "sort", "stats", "runs", "bigsort", "chain", "ovsort", "score", "prefilter", "final", "annotate", "score:quick", "score:banded", "score:finish", "extend:ungapped", "after-extend", "extend:list", "extend:dp4", "extend:dp1", "extend:combine", "seed:replay", "seed:scan", "extend:launch", "-", "-", "-", "-", "-", "-", "-"};
      unsigned long long tot = 0;
      for (int i = 0; i < T4_NPHASE; ++i) tot += ph[i];
      for (int i = 0; i < T4_NPHASE; ++i) if (ph[i]) fprintf(stderr, "phase %-16s %-7s %6.2f%%  %.3e cycles\n", names[i & 31], i < 32 ? "lds" : "global", 100.0 * (double)ph[i] / (double)tot, (double)ph[i]);
    }
    static unsigned long long cls[4 * T4_NPHASE];
    if (hipMemcpyFromSymbol(cls, HIP_SYMBOL(t4k::g_phaseByOverlaps), sizeof(cls)) == hipSuccess) {
      static const char *names[32] = {"other", "seed:lookup", "expand", "sort", "stats", "runs", "bigsort", "chain", "ovsort", "score", "prefilter", "final", "annotate", "score:quick", "score:banded", "score:finish", "extend:ungapped", "after-extend", "extend:list", "extend:dp4", "extend:dp1", "extend:combine", "seed:replay", "seed:scan", "extend:launch", "-", "-", "-", "-", "-", "-", "-"};
      static const char *cname[4] = {"<5 overlaps", "5-19 overlaps", "20-64 overlaps", ">64 overlaps"};
      for (int k = 0; k < 4; ++k) {
        unsigned long long tot = 0;
        for (int i = 0; i < T4_NPHASE; ++i) tot += cls[k * T4_NPHASE + i];
        if (!tot) continue;
        fprintf(stderr, "AddRead queries with %s: %.3e cycles in the query kernel\n", cname[k], (double)tot);
        for (int i = 0; i < T4_NPHASE; ++i) if (cls[k * T4_NPHASE + i] * 200 >= tot) fprintf(stderr, "   %-16s %-7s %6.2f%%\n", names[i & 31], i < 32 ? "lds" : "global", 100.0 * (double)cls[k * T4_NPHASE + i] / (double)tot);
      }
    }
    unsigned long long dc[8];
    if (hipMemcpyFromSymbol(dc, HIP_SYMBOL(t4k::g_dbgCount), sizeof(dc)) == hipSuccess)
      fprintf(stderr, "debug counters: gap jobs %llu, banded %llu, wave-DP steps %llu, scratch fallbacks %llu; overhang DPs %llu, of which %llu leave the diagonal\n", dc[0], dc[1], dc[2], dc[3], dc[6], dc[7]);
  }
#endif
  delete c;
}

int t4_sync(t4_ctx *c) {
  if (!c) return T4_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return T4_OK;
}
const char *t4_last_error(t4_ctx *c) { return c ? c->err.c_str() : "null ctx"; }
int t4_device_cus(t4_ctx *c) { return c ? c->cus : 0; }
int t4_ctx_device(t4_ctx *c) { return c ? c->device : 0; }
#ifdef T4_PHASE_TIMING
// development aid: cycles spent per kernel phase (summed over workgroups) since the last call
int t4_debug_phase_cycles(unsigned long long *out16) {   // T4_NPHASE entries
  unsigned long long zero[T4_NPHASE] = {0};
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(t4k::g_phaseCycles), sizeof(zero)) != hipSuccess) return T4_ERR_HIP;
  if (hipMemcpyToSymbol(HIP_SYMBOL(t4k::g_phaseCycles), zero, sizeof(zero)) != hipSuccess) return T4_ERR_HIP;
  return T4_OK;
}
int t4_debug_counters(unsigned long long *out8) {
  unsigned long long zero[8] = {0};
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(t4k::g_dbgCount), sizeof(zero)) != hipSuccess) return T4_ERR_HIP;
  if (hipMemcpyToSymbol(HIP_SYMBOL(t4k::g_dbgCount), zero, sizeof(zero)) != hipSuccess) return T4_ERR_HIP;
  return T4_OK;
}
#endif
// development aid (T4_PHASE_TIMING builds): forget the phase cycles counted so far; a no-op otherwise
int t4_debug_phase_reset(void) {
#ifdef T4_PHASE_TIMING
  unsigned long long zero[T4_NPHASE] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(t4k::g_phaseCycles), zero, sizeof(zero)) != hipSuccess) return T4_ERR_HIP;
#endif
  return T4_OK;
}
int t4_last_stats(t4_ctx *c, t4_stats *out) {
  if (!c || !out) return T4_ERR_ARG;
  *out = c->stats;
  return T4_OK;
}

// ---- index -------------------------------------------------------------------------------------
int t4_index_create(t4_ctx *c, int k, int consider_barcode, t4_index **out) {
  if (!c || !out) return T4_ERR_ARG;
  if (k < 2 || k > 31) return fail(c, T4_ERR_ARG, "kmer_length %d outside [2,31]", k);
  t4_index *ix = new t4_index();
  ix->ctx = c; ix->k = k; ix->considerBarcode = consider_barcode ? 1 : 0;
  double kmerHitProb = pow(0.8, k);  // SeqSet::ComputeNomatchGapLimit (SeqSet.hpp:2476-2482)
  ix->nomatchGapLimit = int(k * (log(0.01) / log(1 - kmerHitProb))) + 1;
  *out = ix;
  return T4_OK;
}

void t4_index_destroy(t4_index *ix) {
  if (!ix) return;
  if (ix->live) (void)hipStreamSynchronize(ix->ctx->stream);
  delete ix;
}

int t4_index_set_params(t4_index *ix, int hit_len_required, int radius, double novel_sim) {
  if (!ix) return T4_ERR_ARG;
  ix->hitLenRequired = hit_len_required; ix->radius = radius; ix->novelSim = novel_sim;
  if (ix->committed) { ix->view.hitLenRequired = hit_len_required; ix->view.radius = radius; ix->view.novelSim = novel_sim; }
  return T4_OK;
}

int t4_index_add_ref_record(t4_index *ix, const char *id, const char *seq, int *seq_id) {
  if (!ix || !id || !seq) return T4_ERR_ARG;
  if (ix->committed) return fail(ix->ctx, T4_ERR_STATE, "index already committed");
  if (seq_id) *seq_id = -1;
  if (strlen(id) < 4) return fail(ix->ctx, T4_ERR_ARG, "gene name '%s' shorter than 4 characters", id);
  if (geneType(id) != 1) {  // drop "/OR" orphon genes unless they are D genes
    for (const char *p = id; *p; ++p)
      if (p[0] == '/' && p[1] == 'O' && p[2] == 'R') return T4_OK;
  }
  std::string cons;
  for (const char *p = seq; *p; ++p) {
    if (*p == '.') continue;
    int c = (signed char)*p;
    if (c >= 'a' && c <= 'z') c = (signed char)(c - ('a' + 'A'));  // reference arithmetic: lower case becomes N
    if (c >= 'A' && c <= 'Z') { if (nucNum((char)c) == -1 && c != 'N') c = 'N'; }
    else c = 'N';
    cons.push_back((char)c);
  }
  auto it = ix->dedup.find(cons);
  if (it != ix->dedup.end()) {
    HostSeq &e = ix->seqs[it->second];
    if (e.name.find(id) == std::string::npos) e.name += std::string("|") + id;
    return T4_OK;
  }
  if ((int)ix->seqs.size() >= T4_MAX_SEQS || (int)cons.size() >= T4_MAX_SEQLEN) return fail(ix->ctx, T4_ERR_UNSUPPORTED, "sequence set too large");
  HostSeq hs;
  hs.name = id; hs.cons = cons; hs.barcode = -1; hs.isRef = true;
  ix->dedup[cons] = (int)ix->seqs.size();
  if (seq_id) *seq_id = (int)ix->seqs.size();
  ix->seqs.push_back(hs);
  return T4_OK;
}

int t4_index_load_ref_fasta(t4_index *ix, const char *path) {
  if (!ix || !path) return T4_ERR_ARG;
  gzFile fp = gzopen(path, "rb");
  if (!fp) return fail(ix->ctx, T4_ERR_IO, "cannot open %s", path);
  std::string id, seq;
  bool have = false;
  std::vector<char> line(1 << 20);
  int rc = T4_OK;
  auto flush = [&]() { if (have && rc == T4_OK) rc = t4_index_add_ref_record(ix, id.c_str(), seq.c_str(), nullptr); };
  while (gzgets(fp, line.data(), (int)line.size())) {
    size_t l = strlen(line.data());
    while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r')) line[--l] = 0;
    if (line[0] == '>') {
      flush();
      size_t i = 1;
      while (line[i] && line[i] != ' ' && line[i] != '\t') ++i;
      id.assign(line.data() + 1, i - 1);
      size_t n = id.size();  // ReadFiles.hpp:180-185 strips a trailing /1 or /2
      if (n >= 2 && (id[n - 1] == '1' || id[n - 1] == '2') && id[n - 2] == '/') id.resize(n - 2);
      seq.clear(); have = true;
    } else if (have) seq.append(line.data(), l);
  }
  flush();
  gzclose(fp);
  return rc;
}

int t4_index_add_contig(t4_index *ix, const char *name, const char *consensus, int barcode, const int32_t *posweight, int *seq_id) {
  if (!ix || !name || !consensus) return T4_ERR_ARG;
  if (ix->committed) return fail(ix->ctx, T4_ERR_STATE, "index already committed");
  HostSeq hs;
  hs.name = name; hs.cons = consensus; hs.barcode = barcode; hs.isRef = false;
  size_t len = hs.cons.size();
  if ((int)ix->seqs.size() >= T4_MAX_SEQS || (int)len >= T4_MAX_SEQLEN) return fail(ix->ctx, T4_ERR_UNSUPPORTED, "sequence set too large");
  for (char ch : hs.cons) if (nucNum(ch) < 0 && ch != 'N') return fail(ix->ctx, T4_ERR_UNSUPPORTED, "contig alphabet must be ACGTN");
  hs.pw.assign(4 * len, 0);
  if (posweight) memcpy(hs.pw.data(), posweight, sizeof(int32_t) * 4 * len);
  else for (size_t i = 0; i < len; ++i) if (hs.cons[i] != 'N') hs.pw[4 * i + nucNum(hs.cons[i])] = 1;
  if (seq_id) *seq_id = (int)ix->seqs.size();
  ix->seqs.push_back(std::move(hs));
  return T4_OK;
}

}  // extern "C"

namespace {
struct Rec { unsigned long long code; int h; int idx, off; };
int commitWithPostings(t4_index *ix, std::vector<Rec> &recs);
}  // namespace

extern "C" {

int t4_index_clear(t4_index *ix) {
  if (!ix) return T4_ERR_ARG;
  ix->seqs.clear(); ix->dedup.clear(); ix->committed = false;
  return T4_OK;
}

int t4_index_commit_postings(t4_index *ix, int64_t n, const uint64_t *code, const int32_t *bucket, const int32_t *idx, const int32_t *offset) {
  if (!ix || n < 0 || (n > 0 && (!code || !bucket || !idx || !offset))) return T4_ERR_ARG;
  std::vector<Rec> recs((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (idx[i] < 0 || idx[i] >= (int)ix->seqs.size()) return fail(ix->ctx, T4_ERR_ARG, "posting %lld names sequence %d", (long long)i, idx[i]);
    recs[(size_t)i] = {code[i], bucket[i], idx[i], offset[i]};
  }
  return commitWithPostings(ix, recs);
}

int t4_index_commit(t4_index *ix) {
  if (!ix) return T4_ERR_ARG;
  const int K = ix->k;
  const unsigned long long mask = K < 32 ? ((1ull << (2 * K)) - 1ull) : ~0ull;
  // postings in BuildIndexFromRead order (KmerIndex.hpp:118-141), keyed by (code, bucket)
  std::vector<Rec> recs;
  for (size_t id = 0; id < ix->seqs.size(); ++id) {
    const HostSeq &s = ix->seqs[id];
    int len = (int)s.cons.size();
    if (len < K) continue;
    unsigned long long code = 0, prev = 0;
    int invalidPos = -1;
    for (int i = 0; i < len; ++i) {
      char ch = s.cons[i];
      if (invalidPos != -1) ++invalidPos;
      code = ((code << 2) & mask) | (unsigned long long)(nucNum(ch) & 3);
      if (ch == 'N') invalidPos = 0;
      if (invalidPos >= K) invalidPos = -1;
      if (i < K - 1) continue;
      if (invalidPos == -1 && (i == K || code != prev)) {
        int h = (int)((code + (unsigned long long)(long long)(ix->considerBarcode ? s.barcode + 1 : 0)) % 1000003ull);
        recs.push_back({code, h, (int)id, i - K + 1});
      }
      prev = code;
    }
  }
  return commitWithPostings(ix, recs);
}

}  // extern "C"

namespace {
int commitWithPostings(t4_index *ix, std::vector<Rec> &recs) {
  t4_ctx *c = ix->ctx;
  (void)hipSetDevice(c->device);
  const int K = ix->k;
  std::stable_sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.code != b.code ? a.code < b.code : a.h < b.h; });
  std::vector<int2> post(recs.size());
  for (size_t i = 0; i < recs.size(); ++i) post[i] = make_int2(recs[i].idx, recs[i].off);
  const bool direct = (K <= 12 && !ix->considerBarcode);
  std::vector<uint2> table;
  std::vector<T4HashEnt> htab;
  unsigned long long hashMask = 0;
  if (direct) {
    table.assign((size_t)1 << (2 * K), make_uint2(0, 0));
    for (size_t i = 0; i < recs.size();) {
      size_t j = i;
      while (j < recs.size() && recs[j].code == recs[i].code) ++j;
      table[recs[i].code] = make_uint2((unsigned)i, (unsigned)(j - i));
      i = j;
    }
  } else {
    size_t nkeys = 0;
    for (size_t i = 0; i < recs.size();) { size_t j = i; while (j < recs.size() && recs[j].code == recs[i].code && recs[j].h == recs[i].h) ++j; ++nkeys; i = j; }
    size_t sz = 1024;
    while (sz < 2 * nkeys + 2) sz <<= 1;
    hashMask = sz - 1;
    T4HashEnt empty; empty.code = 0; empty.h = -1; empty.start = 0; empty.cnt = 0; empty.pad = 0;
    htab.assign(sz, empty);
    for (size_t i = 0; i < recs.size();) {
      size_t j = i;
      while (j < recs.size() && recs[j].code == recs[i].code && recs[j].h == recs[i].h) ++j;
      unsigned long long s = t4k::mix64(recs[i].code * 1000003ull + (unsigned long long)recs[i].h) & hashMask;
      while (htab[s].h >= 0) s = (s + 1) & hashMask;
      htab[s].code = recs[i].code; htab[s].h = recs[i].h; htab[s].start = (unsigned)i; htab[s].cnt = (unsigned)(j - i);
      i = j;
    }
  }
  // sequence table
  std::vector<T4SeqInfo> infos(ix->seqs.size());
  std::string cons;
  std::vector<T4PW> pw;
  bool hasNovel = false, hasRef = false;
  for (size_t id = 0; id < ix->seqs.size(); ++id) {
    const HostSeq &s = ix->seqs[id];
    T4SeqInfo &f = infos[id];
    memset(&f, 0, sizeof f);
    f.consOff = (int)cons.size(); f.len = (int)s.cons.size(); f.barcode = s.barcode; f.isRef = s.isRef ? 1 : 0;
    cons += s.cons; cons.push_back('\0');
    char nm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    strncpy(nm, s.name.c_str(), 7);
    int gt = geneType(nm);
    f.geneType = gt < 0 ? 255 : (unsigned char)gt;
    f.name0 = (unsigned char)nm[0]; f.name1 = (unsigned char)nm[1]; f.name2 = (unsigned char)nm[2]; f.name3 = (unsigned char)nm[3];
    f.pwOff = -1;
    if (!s.isRef) {
      hasNovel = true;
      f.pwOff = (int)pw.size();
      for (int i = 0; i < f.len; ++i) pw.push_back(t4PwByte(s.pw[4 * i], s.pw[4 * i + 1], s.pw[4 * i + 2], s.pw[4 * i + 3]));
      pw.push_back(t4PwByte(0, 0, 0, 0));
      pw[(size_t)f.pwOff] |= T4_PW_MARK_BAD;   // (an image made here carries no posting marks: a restricted re-query reads the posting lists instead, t4_kernels.h expandHitsContig)
    }
  }
  int r;
  ix->dTable.free(); ix->dHtab.free(); ix->dPost.free(); ix->dSeqs.free(); ix->dCons.free(); ix->dPw.free();   // (an image of the other table form leaves none of its arrays)
  if ((r = ix->dPost.alloc(c, post.size()))) return r;
  if ((r = ix->dSeqs.alloc(c, infos.size()))) return r;
  if ((r = ix->dCons.alloc(c, cons.size() + 16))) return r;
  if ((r = ix->dPw.alloc(c, pw.size()))) return r;
  if (direct) { if ((r = ix->dTable.alloc(c, table.size()))) return r; }
  else { if ((r = ix->dHtab.alloc(c, htab.size()))) return r; }
  if (!post.empty()) HIPCHK(c, hipMemcpy(ix->dPost, post.data(), sizeof(int2) * post.size(), hipMemcpyHostToDevice));
  if (!infos.empty()) HIPCHK(c, hipMemcpy(ix->dSeqs, infos.data(), sizeof(T4SeqInfo) * infos.size(), hipMemcpyHostToDevice));
  if (!cons.empty()) HIPCHK(c, hipMemcpy(ix->dCons, cons.data(), cons.size(), hipMemcpyHostToDevice));
  if (!pw.empty()) HIPCHK(c, hipMemcpy(ix->dPw, pw.data(), sizeof(T4PW) * pw.size(), hipMemcpyHostToDevice));
  if (direct) HIPCHK(c, hipMemcpy(ix->dTable, table.data(), sizeof(uint2) * table.size(), hipMemcpyHostToDevice));
  else HIPCHK(c, hipMemcpy(ix->dHtab, htab.data(), sizeof(T4HashEnt) * htab.size(), hipMemcpyHostToDevice));
  T4IndexView &v = ix->view;
  memset(&v, 0, sizeof v);
  v.k = K; v.nseq = (int)ix->seqs.size(); v.direct = direct ? 1 : 0; v.considerBarcode = ix->considerBarcode;
  v.hashMask = hashMask; v.table = ix->dTable; v.htab = ix->dHtab; v.post = ix->dPost; v.seqs = ix->dSeqs;
  v.cons = ix->dCons; v.pw = ix->dPw;
  v.radius = ix->radius; v.hitLenRequired = ix->hitLenRequired; v.nomatchGapLimit = ix->nomatchGapLimit;
  v.firstIsRef = (!ix->seqs.empty() && ix->seqs[0].isRef) ? 1 : 0;
  for (const HostSeq &q : ix->seqs) if (q.isRef) { hasRef = true; break; }
  v.hasNovel = hasNovel ? (hasRef ? 1 : 2) : 0;
  { int maxLen = 0; for (const HostSeq &q : ix->seqs) if ((int)q.cons.size() > maxLen) maxLen = (int)q.cons.size(); v.key32 = t4Key32Bits(v.nseq, maxLen); }
  v.novelSim = ix->novelSim; v.refSim = ix->refSim; v.repeatSim = ix->repeatSim;
  ix->committed = true;
  return T4_OK;
}
}  // namespace

// ---- live set: patch the device image (see trust4_hip.h) ----------------------------------------------------------
extern "C" {

int t4_index_apply_delta(t4_index *ix, const t4_index_delta *d) {
  if (!ix || !d) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  (void)hipSetDevice(c->device);
  if (ix->considerBarcode) return fail(c, T4_ERR_ARG, "t4_index_apply_delta: the index of a live set is not keyed by barcode");
  if (!ix->live && (!ix->seqs.empty() || ix->committed)) return fail(c, T4_ERR_STATE, "t4_index_apply_delta on an index that was filled through t4_index_add_*");
  if (d->table_slots < 2 || (d->table_slots & (d->table_slots - 1))) return fail(c, T4_ERR_ARG, "table_slots must be a power of two");
  if (d->nseq < 0 || d->nseq > T4_MAX_SEQS) return fail(c, T4_ERR_UNSUPPORTED, "more than %d sequences", T4_MAX_SEQS);
  if (d->max_seq_len > T4_MAX_SEQLEN) return fail(c, T4_ERR_UNSUPPORTED, "contig longer than %d", T4_MAX_SEQLEN);
  if (d->post_cap > 0xFFFFFFFFll) return fail(c, T4_ERR_UNSUPPORTED, "more than 2^32 postings");
  int r;
  HIPCHK(c, ix->stEvent.create());
  // capacities
  if (d->table_slots != ix->capTable || d->table_rebuilt) {
    if (d->table_slots != ix->capTable) {
      if (ix->dCtab) HIPCHK(c, hipStreamSynchronize(c->stream));
      ix->capTable = 0;
      if ((r = ix->dCtab.alloc(c, (size_t)d->table_slots))) return r;
      ix->capTable = d->table_slots;
    }
    HIPCHK(c, hipMemsetAsync(ix->dCtab, 0xFF, sizeof(T4HashEntC) * (size_t)ix->capTable, c->stream));   // code ~0 = empty
  }
  if (d->post_cap > ix->capPost) { int64_t want = d->post_cap + d->post_cap / 2; if ((r = ix->dPost.growKeep(c, ix->capPost, want))) return r; ix->capPost = want; }
  if (d->seq_cap > ix->capSeq) { int want = d->seq_cap + d->seq_cap / 2; if ((r = ix->dSeqs.growKeep(c, (int64_t)ix->capSeq, (int64_t)want))) return r; ix->capSeq = want; }
  if (d->base_cap > ix->capBase) {
    int64_t want = d->base_cap + d->base_cap / 2;
    if ((r = ix->dCons.growKeep(c, ix->capBase, want))) return r;
    if ((r = ix->dPw.growKeep(c, ix->capBase, want))) return r;
    ix->capBase = want;
  }
  // staging: descriptors, then the payload (8-byte aligned pieces)
  auto al8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
  int64_t postTotal = 0, baseTotal = 0;
  for (int64_t i = 0; i < d->n_post_runs; ++i) {
    if (d->post_at[i] < 0 || d->post_len[i] < 0 || d->post_at[i] + d->post_len[i] > ix->capPost) return fail(c, T4_ERR_ARG, "posting run %lld outside the image", (long long)i);
    postTotal += d->post_len[i];
  }
  for (int64_t i = 0; i < d->n_base_runs; ++i) {
    if (d->base_at[i] < 0 || d->base_len[i] < 0 || d->base_at[i] + d->base_len[i] > ix->capBase) return fail(c, T4_ERR_ARG, "base run %lld outside the image", (long long)i);
    baseTotal += d->base_len[i];
  }
  const size_t nDesc = (size_t)d->n_slots + (size_t)d->n_post_runs + (size_t)d->n_seqs + 2 * (size_t)d->n_base_runs;
  if (nDesc == 0) goto view;
  {
    size_t bytes = al8(sizeof(T4CopyDesc) * nDesc) + sizeof(T4HashEntC) * (size_t)d->n_slots + 8 * (size_t)postTotal + al8(sizeof(T4SeqInfo)) * (size_t)d->n_seqs;
    for (int64_t i = 0; i < d->n_base_runs; ++i) bytes += 2 * al8((size_t)d->base_len[i]);
    // the staging buffer is free once the copy that read it is done: a wait for the stream since then (every query round ends with
    // one) says so without an event of its own; two deltas with no wait in between (query lanes) take the wait here
    if (ix->stPending && ix->stEpoch == c->syncEpoch) { HIPCHK(c, hipStreamSynchronize(c->stream)); ++c->syncEpoch; }
    ix->stPending = false;
    if (bytes > ix->stCap) {
      const size_t ncap = bytes * 2 > ((size_t)1 << 20) ? bytes * 2 : ((size_t)1 << 20);
      if (ix->stDev) HIPCHK(c, hipStreamSynchronize(c->stream));
      ix->stCap = 0;
      if ((r = ix->stHost.alloc(c, ncap, hipHostMallocMapped)) || (r = ix->stDev.alloc(c, ncap))) return r;
      ix->stCap = ncap;
    }
    T4CopyDesc *desc = (T4CopyDesc *)ix->stHost.p;
    size_t at = al8(sizeof(T4CopyDesc) * nDesc), nd = 0;
    for (int64_t i = 0; i < d->n_slots; ++i) {
      if (d->slot[i] < 0 || d->slot[i] >= ix->capTable) return fail(c, T4_ERR_ARG, "table slot %lld outside the table", (long long)d->slot[i]);
      T4HashEntC e; e.code = d->slot_code[i]; e.start = d->slot_start[i]; e.cnt = d->slot_cnt[i];
      memcpy(ix->stHost + at, &e, sizeof e);
      desc[nd].srcOff = at; desc[nd].dst = (unsigned char *)(ix->dCtab + d->slot[i]); desc[nd].bytes = sizeof e; ++nd;
      at += sizeof e;
    }
    int64_t pAt = 0;
    for (int64_t i = 0; i < d->n_post_runs; ++i) {
      const size_t b = 8 * (size_t)d->post_len[i];
      memcpy(ix->stHost + at, d->post_data + 2 * pAt, b);
      desc[nd].srcOff = at; desc[nd].dst = (unsigned char *)(ix->dPost + d->post_at[i]); desc[nd].bytes = b; ++nd;
      at += b; pAt += d->post_len[i];
    }
    for (int i = 0; i < d->n_seqs; ++i) {
      const int id = d->seq_id[i];
      if (id < 0 || id >= ix->capSeq || id >= d->nseq) return fail(c, T4_ERR_ARG, "sequence id %d outside the image", id);
      const t4_seq_record &q = d->seq[i];
      if (q.len < 0 || q.base_off < 0 || q.base_off + q.len + 1 > ix->capBase || q.base_off > 0x7FFFFFFFll) return fail(c, T4_ERR_ARG, "sequence %d outside the base arena", id);
      T4SeqInfo f;
      memset(&f, 0, sizeof f);
      f.consOff = (int)q.base_off; f.len = q.len; f.pwOff = (int)q.base_off; f.barcode = q.barcode; f.isRef = 0;
      char nm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      memcpy(nm, q.name, 8);
      const int gt = geneType(nm);
      f.geneType = gt < 0 ? 255 : (unsigned char)gt;
      f.name0 = (unsigned char)nm[0]; f.name1 = (unsigned char)nm[1]; f.name2 = (unsigned char)nm[2]; f.name3 = (unsigned char)nm[3];
      memset(ix->stHost + at, 0, al8(sizeof f));
      memcpy(ix->stHost + at, &f, sizeof f);
      desc[nd].srcOff = at; desc[nd].dst = (unsigned char *)(ix->dSeqs + id); desc[nd].bytes = sizeof f; ++nd;
      at += al8(sizeof f);
    }
    int64_t bAt = 0;
    for (int64_t i = 0; i < d->n_base_runs; ++i) {
      const size_t b = (size_t)d->base_len[i];
      memcpy(ix->stHost + at, d->base_cons + bAt, b);
      desc[nd].srcOff = at; desc[nd].dst = (unsigned char *)(ix->dCons + d->base_at[i]); desc[nd].bytes = b; ++nd;
      at += al8(b);
      memcpy(ix->stHost + at, d->base_pw + bAt, b);
      desc[nd].srcOff = at; desc[nd].dst = (unsigned char *)(ix->dPw + d->base_at[i]); desc[nd].bytes = b; ++nd;
      at += al8(b);
      bAt += d->base_len[i];
    }
    // A round's delta is a few kilobytes: the kernel reads descriptors and payload straight out of the pinned staging buffer (one
    // stream operation; an H2D copy in front of it was a hop to a copy engine and back on the ordered chain's critical path). The
    // whole image of a fresh set, or a rebuilt table, goes through the copy engine as before.
    const bool direct = at <= ((size_t)1 << 18);
    if (!direct) HIPCHK(c, hipMemcpyAsync(ix->stDev, ix->stHost, at, hipMemcpyHostToDevice, c->stream));
    ix->stPending = true; ix->stEpoch = c->syncEpoch;
    int grid = (int)((nd + 3) / 4);
    if (grid > c->cus * 8) grid = c->cus * 8;
    const unsigned char *stg = direct ? ix->stHost.dev : ix->stDev.p;
    hipLaunchKernelGGL(t4k::deltaKernel, dim3(grid), dim3(256), 0, c->stream, stg, (const T4CopyDesc *)stg, (int)nd);
    HIPCHK(c, hipGetLastError());
  }
view:
  ix->live = true; ix->committed = true; ix->liveNseq = d->nseq;
  T4IndexView &v = ix->view;
  memset(&v, 0, sizeof v);
  v.k = ix->k; v.nseq = d->nseq; v.direct = 3; v.considerBarcode = 0;
  v.hashMask = (unsigned long long)ix->capTable - 1; v.ctab = ix->dCtab; v.post = ix->dPost; v.seqs = ix->dSeqs; v.cons = ix->dCons; v.pw = ix->dPw;
  v.radius = ix->radius; v.hitLenRequired = ix->hitLenRequired; v.nomatchGapLimit = ix->nomatchGapLimit;
  v.firstIsRef = 0; v.hasNovel = 2;
  v.key32 = t4Key32Bits(d->nseq, d->max_seq_len);
  v.novelSim = ix->novelSim; v.refSim = ix->refSim; v.repeatSim = ix->repeatSim;
  return T4_OK;
}

int t4_index_size(const t4_index *ix) { return ix ? (ix->live ? ix->liveNseq : (int)ix->seqs.size()) : 0; }
int t4_index_seq_len(const t4_index *ix, int i) { return (ix && i >= 0 && i < (int)ix->seqs.size()) ? (int)ix->seqs[i].cons.size() : -1; }
const char *t4_index_seq_name(const t4_index *ix, int i) { return (ix && i >= 0 && i < (int)ix->seqs.size()) ? ix->seqs[i].name.c_str() : nullptr; }
const char *t4_index_seq_consensus(const t4_index *ix, int i) { return (ix && i >= 0 && i < (int)ix->seqs.size()) ? ix->seqs[i].cons.c_str() : nullptr; }

// ---- reads -------------------------------------------------------------------------------------
int t4_reads_upload(t4_ctx *c, const char *bases, const int64_t *offsets, const int32_t *barcode, int64_t n, t4_batch **out) {
  return t4_reads_upload_flags(c, bases, offsets, barcode, n, 0, out);
}

int t4_reads_upload_flags(t4_ctx *c, const char *bases, const int64_t *offsets, const int32_t *barcode, int64_t n, int flags, t4_batch **out) {
  if (!c || !out || n < 0 || (n > 0 && (!bases || !offsets))) return T4_ERR_ARG;
  *out = nullptr;
  (void)hipSetDevice(c->device);
  int maxLen = 0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t l = offsets[i + 1] - offsets[i];
    if (l < 0) return fail(c, T4_ERR_ARG, "offsets not monotone at read %lld", (long long)i);
    if (l > T4_MAXL) return fail(c, T4_ERR_UNSUPPORTED, "read %lld is %lld bp; this engine takes reads up to %d bp", (long long)i, (long long)l, T4_MAXL);
    if (l > maxLen) maxLen = (int)l;
  }
  std::unique_ptr<t4_batch> b(new t4_batch());   // (and its device buffers, on every way out but the last)
  b->ctx = c; b->n = n; b->maxLen = maxLen;
  b->wpk = (maxLen + 15) / 16; b->wnm = (maxLen + 31) / 32;
  if (b->wpk == 0) b->wpk = 1;
  if (b->wnm == 0) b->wnm = 1;
  std::vector<unsigned> pk((size_t)n * b->wpk, 0u), nm((size_t)n * b->wnm, 0u);
  std::vector<int> len((size_t)n);
  // 2-bit packing on a few host threads for large batches (a million reads: 0.2 s on one thread, more than their kernels take)
  std::atomic<long long> badRead(-1);
  auto packRange = [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      const char *s = bases + offsets[i];
      int l = (int)(offsets[i + 1] - offsets[i]);
      len[i] = l;
      unsigned *p = pk.data() + (size_t)i * b->wpk, *m = nm.data() + (size_t)i * b->wnm;
      for (int j = 0; j < l; ++j) {
        int v = nucNum(s[j]);
        if (v < 0) {
          if (s[j] == 'N') { m[j >> 5] |= 1u << (j & 31); v = 0; }
          else if ((flags & T4_READS_KMERS_ONLY) && s[j] >= 'A' && s[j] <= 'Z') v = 3;   // nucToNum[c - 'A'] & 3 of KmerCode::Append (KmerCode.hpp:99-106): a valid 'T'
          else { long long none = -1; badRead.compare_exchange_strong(none, (long long)i); return; }
        }
        p[j >> 4] |= (unsigned)v << ((j & 15) * 2);
      }
    }
  };
  {
    const int packThreads = getenv("T4_PACK_THREADS") ? atoi(getenv("T4_PACK_THREADS")) : 8;
    const long long packMin = getenv("T4_PACK_MIN") ? atoll(getenv("T4_PACK_MIN")) : 65536;   // testing aid: threads for small batches too
    int nt = n >= packMin ? packThreads : 1;
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw > 0 && (unsigned)nt > hw) nt = (int)hw;
    if (nt <= 1) packRange(0, n);
    else {
      std::vector<std::thread> pool;
      for (int t = 0; t < nt; ++t) pool.emplace_back(packRange, n * t / nt, n * (t + 1) / nt);
      for (auto &th : pool) th.join();
    }
  }
  if (badRead.load() >= 0) {
    const long long i = badRead.load();
    char bad = '?';
    for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) { const char ch = bases[j]; if (nucNum(ch) < 0 && ch != 'N' && !((flags & T4_READS_KMERS_ONLY) && ch >= 'A' && ch <= 'Z')) { bad = ch; break; } }
    return fail(c, T4_ERR_UNSUPPORTED, "read %lld has base '%c' (alphabet is ACGTN)", i, bad);
  }
  int r;
  // + 4 words: the packed k-mer extraction reads one word past a read's row (masked out), also for the last read
  if ((r = b->dPk.alloc(c, pk.size() + 4)) || (r = b->dNm.alloc(c, nm.size() + 4)) || (r = b->dLen.alloc(c, len.size()))) return r;
  if (n > 0) {
    HIPCHK(c, hipMemcpy(b->dPk, pk.data(), sizeof(unsigned) * pk.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(b->dNm, nm.data(), sizeof(unsigned) * nm.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(b->dLen, len.data(), sizeof(int) * len.size(), hipMemcpyHostToDevice));
  }
  if (barcode) {
    if ((r = b->dBarcode.alloc(c, (size_t)n))) return r;
    if (n > 0) HIPCHK(c, hipMemcpy(b->dBarcode, barcode, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    for (int64_t i = 0; i < n; ++i) { if (barcode[i] < b->minBarcode) b->minBarcode = barcode[i]; if (barcode[i] > b->maxBarcode) b->maxBarcode = barcode[i]; }
  }
  b->view.pk = b->dPk; b->view.nm = b->dNm; b->view.len = b->dLen; b->view.barcode = b->dBarcode;
  b->view.wpk = b->wpk; b->view.wnm = b->wnm; b->view.n = n;
  *out = b.release();
  return T4_OK;
}

void t4_batch_destroy(t4_batch *b) { delete b; }
int64_t t4_batch_size(const t4_batch *b) { return b ? b->n : 0; }

}  // extern "C"

namespace {

template <int CAP, int MAXOV, int NT>
void launchTier(int grid, hipStream_t st, const T4IndexView &iv, const T4BatchView &bv, const T4Work &wk, const T4QueryArgs &qa) {
  if (qa.views) hipLaunchKernelGGL((t4k::queryKernel<CAP, MAXOV, NT, 2>), dim3(grid), dim3(NT), 0, st, iv, bv, wk, qa);
  else if (qa.mode == 5) hipLaunchKernelGGL((t4k::queryKernel<CAP, MAXOV, NT, 3>), dim3(grid), dim3(NT), 0, st, iv, bv, wk, qa);
  else if (qa.mode >= 2 && qa.mode <= 4) hipLaunchKernelGGL((t4k::queryKernel<CAP, MAXOV, NT, 1>), dim3(grid), dim3(NT), 0, st, iv, bv, wk, qa);
  else hipLaunchKernelGGL((t4k::queryKernel<CAP, MAXOV, NT, 0>), dim3(grid), dim3(NT), 0, st, iv, bv, wk, qa);
}

// Shared driver of t4_overlaps / t4_annotate_rough. statusOut (nullable): the per-read status words are handed back instead of turned
// into a refusal -- the rows of the reads with status 0 are final, the caller answers the others another way (t4_assign_wide).
int runQuery(t4_index *ix, t4_batch *b, T4QueryArgs qa, bool useBarcode, bool noHits = false, std::vector<int> *statusOut = nullptr) {
  t4_ctx *c = ix->ctx;
  if (!ix->committed) return fail(c, T4_ERR_STATE, "index not committed");
  if (b->ctx != c) return fail(c, T4_ERR_ARG, "batch belongs to another ctx");
  (void)hipSetDevice(c->device);
  const long long n = b->n;
  memset(&c->stats, 0, sizeof c->stats);
  c->stats.reads = n;
  if (n == 0) return T4_OK;
  int r;
  int grids[T4_NTIER];
  int maxGrid = 1;
  for (int t = 0; t < T4_NTIER; ++t) {
    grids[t] = c->cus * TIER_BLOCKS_PER_CU[t];
    if (grids[t] * TIER_THREADS[t] > maxGrid) maxGrid = grids[t] * TIER_THREADS[t];
  }
  if ((r = ensureScratch(c, maxGrid))) return r;
  if ((r = ensurePerCall(c, n))) return r;
  HIPCHK(c, hipMemsetAsync(c->listCounts, 0, sizeof(int) * 16, c->stream));   // [0..8) tier counts, [8..16) tier work counters
  HIPCHK(c, hipMemsetAsync(c->status, 0, sizeof(int) * (size_t)n, c->stream));
  HIPCHK(c, hipMemsetAsync(c->hitCounter, 0, sizeof(unsigned long long), c->stream));
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  T4TierCaps caps;
  for (int t = 0; t < T4_NTIER - 1; ++t) caps.cap[t] = TIER_CAP[t];
  if (noHits) caps.cap[0] = 1 << 30;
  int binGrid = c->cus * 8;
  if ((long long)binGrid > n) binGrid = (int)n;
  hipLaunchKernelGGL(t4k::binKernel, dim3(binGrid), dim3(64), 0, c->stream, ix->view, b->view, useBarcode ? 1 : 0,
                     caps, c->lists, c->listCounts, (long long)n);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  c->stats.launches = 1;
  int hostCounts[8];
  for (int t = 0; t < T4_NTIER; ++t) {
    HIPCHK(c, hipMemcpyAsync(hostCounts, c->listCounts, sizeof(int) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int cnt = hostCounts[t];
    c->stats.tier_reads[t] = cnt;
    if (cnt == 0) continue;
    T4Work wk;
    memset(&wk, 0, sizeof wk);
    wk.list = c->lists + (size_t)t * n; wk.nList = cnt;
    wk.nextList = t + 1 < T4_NTIER ? c->lists + (size_t)(t + 1) * n : nullptr;
    wk.nextCount = t + 1 < T4_NTIER ? c->listCounts + (t + 1) : nullptr;
    wk.workNext = getenv("T4_STATIC_STRIDE") ? nullptr : c->listCounts + 8 + t;   // reads cost very different amounts: blocks fetch their next read
    wk.status = c->status; wk.hitCounter = c->hitCounter;
    wk.dpRows = c->dpRows; wk.dpDir = c->dpDir;
    int grid = grids[t] < cnt ? grids[t] : cnt;
    if (t == T4_NTIER - 1) {
      if ((r = ensureGlobalTier(c, grids[T4_NTIER - 1]))) return r;
      wk.gKeys = c->gKeys; wk.gPairs = c->gPairs; wk.gCand = nullptr; wk.gOv = c->gOv; wk.gFin = c->gFin; wk.gOrd = c->gOrd;
      wk.gCap = G_CAP; wk.gMaxOv = G_MAXOV;
      launchTier<0, 0, G_THREADS>(grid, c->stream, ix->view, b->view, wk, qa);
    }
    // (threads per read and resident groups per CU of every tier: TIER_THREADS / TIER_BLOCKS_PER_CU above; measured in rounds 1-3)
    else if (t == 0) launchTier<1024, 64, 128>(grid, c->stream, ix->view, b->view, wk, qa);
    else if (t == 1) launchTier<2048, 128, 256>(grid, c->stream, ix->view, b->view, wk, qa);
    else if (t == 2) launchTier<3072, 128, 256>(grid, c->stream, ix->view, b->view, wk, qa);
    else if (t == 3) launchTier<4096, 256, 256>(grid, c->stream, ix->view, b->view, wk, qa);
    else launchTier<8192, 512, 512>(grid, c->stream, ix->view, b->view, wk, qa);
    HIPCHK(c, hipGetLastError());
    ++c->stats.launches;
  }
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  std::vector<int> status((size_t)n);
  unsigned long long hits = 0;
  HIPCHK(c, hipMemcpyAsync(status.data(), c->status, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&hits, c->hitCounter, sizeof hits, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float msAll = 0, msChain = 0;
  HIPCHK(c, hipEventElapsedTime(&msAll, c->ev[0], c->ev[2]));
  HIPCHK(c, hipEventElapsedTime(&msChain, c->ev[1], c->ev[2]));
  c->stats.kernel_ms = msAll; c->stats.chain_kernel_ms = msChain; c->stats.total_hits = (int64_t)hits;
  if (statusOut) { statusOut->swap(status); return T4_OK; }
  for (long long i = 0; i < n; ++i)
    if (status[i] != 0)
      return fail(c, T4_ERR_UNSUPPORTED, "read %lld exceeds the engine limits (status %d: %s)", i, status[i],
                  status[i] == 2 ? "more than 262144 k-mer hits or 16384 overlaps" : "a posting list beyond 10000 entries, or gap DP or contig count beyond scratch");
  return T4_OK;
}

int ensureResult(t4_ctx *c, size_t records) {
  if (records <= c->resultCap) return T4_OK;
  c->resultCap = 0;
  int r = c->result.alloc(c, records);
  if (r) return r;
  c->resultCap = records;
  return T4_OK;
}

}  // namespace

extern "C" {

int t4_overlaps(t4_index *ix, t4_batch *b, int strand, int skip_repeats, int max_per_read, int32_t *counts, t4_overlap *out) {
  if (!ix || !b || max_per_read <= 0) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  int r;
  if ((r = ensurePerCall(c, b->n))) return r;
  if ((r = ensureResult(c, (size_t)b->n * max_per_read))) return r;
  T4QueryArgs qa;
  memset(&qa, 0, sizeof qa);
  qa.mode = 0; qa.strand = strand; qa.skipRepeats = skip_repeats; qa.maxPerRead = max_per_read;
  qa.counts = c->counts; qa.out = c->result;
  if ((r = runQuery(ix, b, qa, true))) return r;
  if (counts && b->n) HIPCHK(c, hipMemcpy(counts, c->counts, sizeof(int) * (size_t)b->n, hipMemcpyDeviceToHost));
  if (out && b->n) HIPCHK(c, hipMemcpy(out, c->result, sizeof(t4_overlap) * (size_t)b->n * max_per_read, hipMemcpyDeviceToHost));
  return T4_OK;
}

int t4_annotate_rough(t4_index *ref, t4_batch *b, t4_overlap *out) {
  if (!ref || !b) return T4_ERR_ARG;
  t4_ctx *c = ref->ctx;
  int r;
  if ((r = ensureResult(c, (size_t)b->n * 4))) return r;
  T4QueryArgs qa;
  memset(&qa, 0, sizeof qa);
  qa.mode = 1; qa.strand = 0; qa.skipRepeats = 0; qa.maxPerRead = 4; qa.counts = nullptr; qa.out = c->result;
  if ((r = runQuery(ref, b, qa, false))) return r;
  if (out && b->n) HIPCHK(c, hipMemcpy(out, c->result, sizeof(t4_overlap) * (size_t)b->n * 4, hipMemcpyDeviceToHost));
  return T4_OK;
}

int t4_hits(t4_index *ix, t4_batch *b, int strand, int allow_total_skip, int64_t *hit_offsets, t4_hit *hits, int64_t hits_cap) {
  if (!ix || !b || !hit_offsets) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (!ix->committed) return fail(c, T4_ERR_STATE, "index not committed");
  (void)hipSetDevice(c->device);
  const long long n = b->n;
  hit_offsets[0] = 0;
  if (n == 0) return T4_OK;
  int r;
  int grid = c->cus * 2;
  if ((long long)grid > n) grid = (int)n;
  const int HCAP = 65536;
  if (grid > c->hitsGrid) { c->hitsGrid = 0; if ((r = c->hitsKeys.alloc(c, (size_t)grid * HCAP))) return r; c->hitsGrid = grid; }
  if ((r = ensurePerCall(c, n))) return r;
  DevBuf<long long> dOff;
  DevBuf<T4HitOut> dHits;
  if ((r = dOff.alloc(c, (size_t)n + 1))) return r;
  HIPCHK(c, hipMemsetAsync(c->status, 0, sizeof(int) * (size_t)n, c->stream));
  launch(t4k::hitsKernel, grid, 64, c->stream, ix->view, b->view, strand, allow_total_skip, 0, dOff,
                     (T4HitOut *)nullptr, c->hitsKeys, HCAP, c->status);
  HIPCHK(c, hipGetLastError());
  std::vector<long long> off((size_t)n + 1);
  HIPCHK(c, hipMemcpyAsync(off.data(), dOff, sizeof(long long) * ((size_t)n + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  off[0] = 0;
  for (long long i = 0; i < n; ++i) off[i + 1] += off[i];
  for (long long i = 0; i <= n; ++i) hit_offsets[i] = off[i];
  std::vector<int> status((size_t)n);
  HIPCHK(c, hipMemcpy(status.data(), c->status, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  for (long long i = 0; i < n; ++i) if (status[i]) return fail(c, T4_ERR_UNSUPPORTED, "read %lld has more than %d hits", i, HCAP);
  if (hits) {
    if (hits_cap < off[n]) return fail(c, T4_ERR_ARG, "hits_cap %lld < %lld", (long long)hits_cap, off[n]);
    if ((r = dHits.alloc(c, (size_t)off[n]))) return r;
    HIPCHK(c, hipMemcpyAsync(dOff, off.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
    launch(t4k::hitsKernel, grid, 64, c->stream, ix->view, b->view, strand, allow_total_skip, 1, dOff,
                       dHits, c->hitsKeys, HCAP, c->status);
    HIPCHK(c, hipGetLastError());
    if (off[n]) HIPCHK(c, hipMemcpyAsync(hits, dHits, sizeof(t4_hit) * (size_t)off[n], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return T4_OK;
}


int t4_gap_dp_align(t4_ctx *c, int kind, int impl, int n, const int64_t *t_off, const int64_t *p_off, const void *t_data,
                    const char *p_chars, int32_t *out4, signed char *align, int align_stride);
int t4_gap_dp(t4_ctx *c, int kind, int impl, int n, const int64_t *t_off, const int64_t *p_off, const void *t_data,
              const char *p_chars, int32_t *out4) {
  return t4_gap_dp_align(c, kind, impl, n, t_off, p_off, t_data, p_chars, out4, nullptr, 0);
}
// the same; impl 4 with kind 1 also returns the edit string of every alignment (align_stride bytes each, terminated by -1)
int t4_gap_dp_align(t4_ctx *c, int kind, int impl, int n, const int64_t *t_off, const int64_t *p_off, const void *t_data,
                    const char *p_chars, int32_t *out4, signed char *align, int align_stride) {
  if (!c || n < 0 || (n > 0 && (!t_off || !p_off || !t_data || !p_chars || !out4)) || (kind != 0 && kind != 1)) return T4_ERR_ARG;
  if (align && (align_stride < 2 || impl != 4 || kind != 1)) return T4_ERR_ARG;
  if (n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  int grid = (n + 63) / 64;
  if (grid > c->cus * 4) grid = c->cus * 4;
  int r;
  if ((r = ensureScratch(c, grid * 64))) return r;
  DevBuf<long long> dT, dP;
  DevBuf<char> dTc, dPc;
  DevBuf<T4PW> dTw;
  DevBuf<int> dOut;
  size_t tn = (size_t)t_off[n], pn = (size_t)p_off[n];
  if ((r = dT.alloc(c, (size_t)n + 1)) || (r = dP.alloc(c, (size_t)n + 1)) || (r = dPc.alloc(c, pn + 16)) || (r = dOut.alloc(c, (size_t)n * 4))) return r;
  if (kind == 0) { if ((r = dTc.alloc(c, tn + 16))) return r; HIPCHK(c, hipMemcpy(dTc, t_data, tn, hipMemcpyHostToDevice)); }
  else {   // _posWeight columns (4 x int32) -> predicate bytes
    std::vector<T4PW> wb(tn + 1, t4PwByte(0, 0, 0, 0));
    const int32_t *w4 = (const int32_t *)t_data;
    for (size_t i = 0; i < tn; ++i) wb[i] = t4PwByte(w4[4 * i], w4[4 * i + 1], w4[4 * i + 2], w4[4 * i + 3]);
    if ((r = dTw.alloc(c, tn + 16))) return r;
    HIPCHK(c, hipMemcpy(dTw, wb.data(), tn + 1, hipMemcpyHostToDevice));
  }
  HIPCHK(c, hipMemcpy(dT, t_off, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dP, p_off, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dPc, p_chars, pn, hipMemcpyHostToDevice));
  DevBuf<signed char> dAl;
  if (align) { if ((r = dAl.alloc(c, (size_t)n * align_stride))) return r; HIPCHK(c, hipMemsetAsync(dAl, 0xFF, (size_t)n * align_stride, c->stream)); }
  launch(t4k::gapDpKernel, grid, 64, c->stream, kind, impl, n, dT, dP, dTc, dTw, dPc, dOut, c->dpRows, c->dpDir, dAl, align_stride);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out4, dOut, sizeof(int) * (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (align) HIPCHK(c, hipMemcpyAsync(align, dAl, (size_t)n * align_stride, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return T4_OK;
}


int t4_mate_overlap(t4_ctx *c, int n, const int64_t *f_off, const char *f_chars, const int64_t *s_off, const char *s_chars,
                    const int32_t *min_overlap, int check_tandem, int32_t *out3) {
  if (!c || n < 0 || (n > 0 && (!f_off || !f_chars || !s_off || !s_chars || !min_overlap || !out3))) return T4_ERR_ARG;
  if (n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  int r;
  DevBuf<long long> dF, dS;
  DevBuf<char> dFc, dSc;
  DevBuf<int> dMo, dOut;
  const size_t fn = (size_t)f_off[n], sn = (size_t)s_off[n];
  if ((r = dF.alloc(c, (size_t)n + 1)) || (r = dS.alloc(c, (size_t)n + 1)) || (r = dFc.alloc(c, fn + 16)) ||
      (r = dSc.alloc(c, sn + 16)) || (r = dMo.alloc(c, (size_t)n)) || (r = dOut.alloc(c, (size_t)n * 3))) return r;
  HIPCHK(c, hipMemcpy(dF, f_off, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dS, s_off, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice));
  if (fn) HIPCHK(c, hipMemcpy(dFc, f_chars, fn, hipMemcpyHostToDevice));
  if (sn) HIPCHK(c, hipMemcpy(dSc, s_chars, sn, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dMo, min_overlap, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  int grid = n < c->cus * 32 ? n : c->cus * 32;
  launch(t4k::mateOverlapKernel, grid, 64, c->stream, n, dF, dFc, dS, dSc, dMo, check_tandem ? 1 : 0, dOut);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out3, dOut, sizeof(int) * (size_t)n * 3, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) if (out3[3 * i] == -2) return fail(c, T4_ERR_UNSUPPORTED, "pair %d has a read longer than %d bp", i, T4_MAXL);
  return T4_OK;
}

int t4_process_pairs(t4_ctx *c, int n, const int64_t *off1, const char *r1, const char *q1, const int64_t *off2, const char *r2, const char *q2,
                     const unsigned char *has_qual, const int64_t *out_off, char *out_r, char *out_q, int32_t *meta4) {
  if (!c || n < 0 || (n > 0 && (!off1 || !r1 || !off2 || !r2 || !has_qual || !out_off || !out_r || !out_q || !meta4))) return T4_ERR_ARG;
  if (n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  const size_t n1 = (size_t)off1[n], n2 = (size_t)off2[n], no = (size_t)out_off[n];
  for (int i = 0; i < n; ++i) {
    if (out_off[i + 1] - out_off[i] < (off1[i + 1] - off1[i]) + (off2[i + 1] - off2[i]) + 1) return fail(c, T4_ERR_ARG, "t4_process_pairs: pair %d needs an output slot of len1 + len2 + 1 characters", i);
    if ((has_qual[i] & 1) && !q1) return fail(c, T4_ERR_ARG, "t4_process_pairs: pair %d says read 1 has qualities, q1 is null", i);
    if ((has_qual[i] & 2) && !q2) return fail(c, T4_ERR_ARG, "t4_process_pairs: pair %d says read 2 has qualities, q2 is null", i);
  }
  int r;
  DevBuf<long long> dO1, dO2, dOo;
  DevBuf<char> dR1, dQ1, dR2, dQ2, dOr, dOq;
  DevBuf<unsigned char> dHq;
  DevBuf<int4> dMeta;
  if ((r = dO1.alloc(c, (size_t)n + 1)) || (r = dO2.alloc(c, (size_t)n + 1)) || (r = dOo.alloc(c, (size_t)n + 1)) ||
      (r = dR1.alloc(c, n1 + 16)) || (r = dR2.alloc(c, n2 + 16)) || (r = dOr.alloc(c, no + 16)) || (r = dOq.alloc(c, no + 16)) ||
      (r = dHq.alloc(c, (size_t)n)) || (r = dMeta.alloc(c, (size_t)n)) || (q1 && (r = dQ1.alloc(c, n1 + 16))) || (q2 && (r = dQ2.alloc(c, n2 + 16)))) return r;
  HIPCHK(c, hipMemcpyAsync(dO1, off1, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dO2, off2, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dOo, out_off, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
  if (n1) HIPCHK(c, hipMemcpyAsync(dR1, r1, n1, hipMemcpyHostToDevice, c->stream));
  if (n2) HIPCHK(c, hipMemcpyAsync(dR2, r2, n2, hipMemcpyHostToDevice, c->stream));
  if (q1 && n1) HIPCHK(c, hipMemcpyAsync(dQ1, q1, n1, hipMemcpyHostToDevice, c->stream));
  if (q2 && n2) HIPCHK(c, hipMemcpyAsync(dQ2, q2, n2, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dHq, has_qual, (size_t)n, hipMemcpyHostToDevice, c->stream));
  const int grid = n < c->cus * 32 ? n : c->cus * 32;
  launch(t4k::processPairKernel, grid, 64, c->stream, n, dO1, dR1, dQ1, dO2, dR2, dQ2, dHq, dOo, dOr, dOq, dMeta);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(meta4, dMeta, sizeof(int4) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_r, dOr, no, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_q, dOq, no, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) if (meta4[4 * i] == -2) return fail(c, T4_ERR_UNSUPPORTED, "pair %d has a read longer than %d bp", i, T4_MAXL);
  return T4_OK;
}

// ---- KmerCount (KmerCount.hpp) on the device ------------------------------------------------------------------------
struct t4_kmer_counter {
  t4_ctx *ctx = nullptr;
  T4KmerTable tb{};   // (a kernel argument: plain pointers into the four blocks below)
  DevBuf<unsigned long long> keys;
  DevBuf<unsigned> cnt;
  DevBuf<int> overflow;
  DevBuf<unsigned long long> used;
  unsigned long long slots = 0, maxSlots = 0;
};

namespace {
// a table of `slots` slots (a power of two), zeroed; the counter's small words (overflow flag, used-slot count) stay as they are
int kmerTableAlloc(t4_ctx *c, unsigned long long slots, T4KmerTable &tb, DevBuf<unsigned long long> &keys, DevBuf<unsigned> &cnt) {
  if (keys.alloc(c, slots) || cnt.alloc(c, slots)) { keys.free(); return fail(c, T4_ERR_HIP, "k-mer count table: no device memory for %llu slots", slots); }
  HIPCHK(c, hipMemsetAsync(keys, 0, sizeof(unsigned long long) * slots, c->stream));
  HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(unsigned) * slots, c->stream));
  tb.keys = keys; tb.cnt = cnt; tb.mask = slots - 1;
  return T4_OK;
}
// A per-barcode counter keys a k-mer as code | (barcode + 1) << 42 (kmerAddKernel, kmerStatsKernel): barcode + 1 has the 22 bits
// 42..63, and the key is stored as key + 1, so barcodes -1 (none) .. T4_KMER_COUNT_MAX_BARCODE keep apart. One beyond would fold
// onto another's keys, silently: such a batch is refused. (The extremes were taken on the host when the batch got its barcodes.)
int kmerBarcodesFit(t4_kmer_counter *kc, const t4_batch *b, const char *who) {
  if (!kc->tb.perBarcode || !b->dBarcode) return T4_OK;
  if (b->maxBarcode > T4_KMER_COUNT_MAX_BARCODE || b->minBarcode < -1)
    return fail(kc->ctx, T4_ERR_UNSUPPORTED, "%s: barcode %d in the batch; a per-barcode counter keys barcodes -1..%d (22 bits of the 64-bit key)",
                who, b->maxBarcode > T4_KMER_COUNT_MAX_BARCODE ? b->maxBarcode : b->minBarcode, T4_KMER_COUNT_MAX_BARCODE);
  return T4_OK;
}
// Room for `incoming` more k-mers at a load of at most 0.6: the table is rehashed on the device into one four times as large as
// often as that takes (never beyond the size the caller's max_kmers stands for: then the old behaviour -- a full table fails).
// raiseMax: the incoming k-mers are another read set's (t4_kmer_count_merge without only_present), which the caller's max_kmers at
// create time knew nothing of -- the ceiling moves so that what is there plus what comes fits.
int kmerEnsureRoom(t4_kmer_counter *kc, unsigned long long incoming, bool raiseMax = false) {
  t4_ctx *c = kc->ctx;
  unsigned long long used = 0;
  HIPCHK(c, hipMemcpyAsync(&used, kc->tb.used, sizeof used, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (raiseMax) while ((used + incoming) * 10ull > kc->maxSlots * 6ull && kc->maxSlots < (1ull << 40)) kc->maxSlots <<= 1;
  while (kc->slots < kc->maxSlots && (used + incoming) * 10ull > kc->slots * 6ull) {
    unsigned long long ns = kc->slots * 4ull;
    if (ns > kc->maxSlots) ns = kc->maxSlots;
    T4KmerTable to = kc->tb;
    DevBuf<unsigned long long> keys;   // (the new pair; after the swap below the old one, which goes with these two)
    DevBuf<unsigned> cnt;
    int r;
    if ((r = kmerTableAlloc(c, ns, to, keys, cnt))) return r;
    const unsigned long long blocks = (kc->slots + 255ull) / 256ull;
    const int grid = (int)(blocks < (unsigned long long)c->cus * 16ull ? blocks : (unsigned long long)c->cus * 16ull);
    hipLaunchKernelGGL(t4k::kmerRehashKernel, dim3(grid), dim3(256), 0, c->stream, kc->tb, to);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    kc->keys.swap(keys); kc->cnt.swap(cnt);
    kc->tb = to; kc->slots = ns;
  }
  return T4_OK;
}
}  // namespace

int t4_kmer_count_create(t4_ctx *c, int k, int64_t max_kmers, int per_barcode, t4_kmer_counter **out) {
  if (!c || !out) return T4_ERR_ARG;
  if (k < 1 || k > 31 || max_kmers < 1) return fail(c, T4_ERR_ARG, "t4_kmer_count_create: k in 1..31 and max_kmers >= 1 (got %d, %lld)", k, (long long)max_kmers);
  if (per_barcode && k > 21) return fail(c, T4_ERR_UNSUPPORTED, "t4_kmer_count_create: per-barcode counts take k <= 21 (the barcode shares the 64-bit key)");
  (void)hipSetDevice(c->device);
  unsigned long long maxSlots = 1024;
  while (maxSlots < 2ull * (unsigned long long)max_kmers) maxSlots <<= 1;
  // max_kmers is an upper bound -- every k-mer position of the input -- and a read set repeats itself: a table for all of them was
  // 12 GB for a million pairs. It starts at an eighth of that (at least 4 M slots) and grows as it fills.
  unsigned long long slots = maxSlots / 8ull;
  if (slots < (1ull << 22)) slots = (1ull << 22) < maxSlots ? (1ull << 22) : maxSlots;
#ifdef T4_TEST_KNOBS   // (emulator / test builds only)
  if (getenv("T4_KC_SLOTS")) { slots = 1024; const unsigned long long want = strtoull(getenv("T4_KC_SLOTS"), nullptr, 10); while (slots < want && slots < maxSlots) slots <<= 1; }   // testing aid: a small first table (the growth path)
#endif
  std::unique_ptr<t4_kmer_counter> kc(new t4_kmer_counter);
  kc->ctx = c; kc->slots = slots; kc->maxSlots = maxSlots;
  kc->tb.k = k; kc->tb.perBarcode = per_barcode ? 1 : 0;
  int r = kmerTableAlloc(c, slots, kc->tb, kc->keys, kc->cnt);
  if (r) return r;
  if (kc->overflow.alloc(c, 1) || kc->used.alloc(c, 1)) return fail(c, T4_ERR_HIP, "t4_kmer_count_create: no device memory");
  kc->tb.overflow = kc->overflow; kc->tb.used = kc->used;
  HIPCHK(c, hipMemsetAsync(kc->tb.overflow, 0, sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(kc->tb.used, 0, sizeof(unsigned long long), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = kc.release();
  return T4_OK;
}

void t4_kmer_count_destroy(t4_kmer_counter *kc) { delete kc; }

int t4_kmer_count_add(t4_kmer_counter *kc, t4_batch *b) {
  if (!kc || !b) return T4_ERR_ARG;
  t4_ctx *c = kc->ctx;
  if (b->ctx != c) return fail(c, T4_ERR_ARG, "batch belongs to another ctx");
  if (b->n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  const long long n = b->n;
  if (kc->tb.perBarcode && !b->dBarcode) return fail(c, T4_ERR_ARG, "t4_kmer_count_add: per-barcode counts need a batch uploaded with barcodes");
  if (int fit = kmerBarcodesFit(kc, b, "t4_kmer_count_add")) return fit;
  // in slices of reads whose k-mers (every one new, at worst) leave the table under a load of 0.6; between slices the table grows
  const long long perRead = b->maxLen >= kc->tb.k ? (long long)(b->maxLen - kc->tb.k + 1) : 1;
  for (long long lo = 0; lo < n;) {
    long long cnt = n - lo;
    if (kc->slots < kc->maxSlots) {
      long long fit = (long long)(kc->slots * 3ull / 10ull) / perRead;
      if (fit < 4096) fit = 4096;
      if (cnt > fit) cnt = fit;
      int r = kmerEnsureRoom(kc, (unsigned long long)(cnt * perRead));
      if (r) return r;
    }
    const int grid = (int)(cnt < (long long)c->cus * 32 ? cnt : (long long)c->cus * 32);
    hipLaunchKernelGGL(t4k::kmerAddKernel, dim3(grid), dim3(64), 0, c->stream, b->view, kc->tb, lo, lo + cnt);
    HIPCHK(c, hipGetLastError());
    lo += cnt;
  }
  int overflow = 0;
  HIPCHK(c, hipMemcpyAsync(&overflow, kc->tb.overflow, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (overflow) return fail(c, T4_ERR_UNSUPPORTED, "t4_kmer_count_add: more distinct k-mers than the table was created for (%llu slots)", kc->slots);
  return T4_OK;
}

int t4_kmer_count_set(t4_kmer_counter *kc, const uint64_t *codes, const int32_t *counts, int64_t n) {
  if (!kc || n < 0 || (n > 0 && (!codes || !counts))) return T4_ERR_ARG;
  t4_ctx *c = kc->ctx;
  if (kc->tb.perBarcode) return fail(c, T4_ERR_ARG, "t4_kmer_count_set: not for per-barcode counters");
  if (n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  std::unordered_map<uint64_t, int32_t> last;   // a later record of the same k-mer overwrites an earlier one
  last.reserve((size_t)n * 2);
  for (int64_t i = 0; i < n; ++i) last[codes[i]] = counts[i];
  std::vector<unsigned long long> hc; std::vector<int> hv;
  hc.reserve(last.size()); hv.reserve(last.size());
  for (const auto &kv : last) { hc.push_back((unsigned long long)kv.first); hv.push_back((int)kv.second); }
  const long long m = (long long)hc.size();
  int r;
  if ((r = kmerEnsureRoom(kc, (unsigned long long)m))) return r;
  DevBuf<unsigned long long> dC; DevBuf<int> dV;
  if ((r = dC.alloc(c, (size_t)m)) || (r = dV.alloc(c, (size_t)m))) return r;
  HIPCHK(c, hipMemcpy(dC, hc.data(), sizeof(unsigned long long) * (size_t)m, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dV, hv.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice));
  const int grid = (int)((m + 255) / 256 < (long long)c->cus * 8 ? (m + 255) / 256 : (long long)c->cus * 8);
  launch(t4k::kmerSetKernel, grid, 256, c->stream, kc->tb, (const unsigned long long *)dC, (const int *)dV, m);
  HIPCHK(c, hipGetLastError());
  int overflow = 0;
  HIPCHK(c, hipMemcpyAsync(&overflow, kc->tb.overflow, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (overflow) return fail(c, T4_ERR_UNSUPPORTED, "t4_kmer_count_set: more distinct k-mers than the table was created for (%llu slots)", kc->slots);
  return T4_OK;
}

int t4_kmer_count_export(t4_kmer_counter *kc, uint64_t *codes, int32_t *counts, int64_t cap, int64_t *n_out) {
  if (!kc || !n_out || cap < 0 || (cap > 0 && (!codes || !counts))) return T4_ERR_ARG;
  t4_ctx *c = kc->ctx;
  (void)hipSetDevice(c->device);
  unsigned long long used = 0;
  HIPCHK(c, hipMemcpyAsync(&used, kc->tb.used, sizeof used, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_out = (int64_t)used;
  if (cap == 0 || used == 0) return T4_OK;
  int r;
  DevBuf<unsigned long long> dC, dCur; DevBuf<int> dV;
  if ((r = dC.alloc(c, (size_t)cap)) || (r = dV.alloc(c, (size_t)cap)) || (r = dCur.alloc(c, (size_t)1))) return r;
  HIPCHK(c, hipMemsetAsync(dCur, 0, sizeof(unsigned long long), c->stream));
  const unsigned long long blocks = (kc->slots + 255ull) / 256ull;
  const int grid = (int)(blocks < (unsigned long long)c->cus * 16ull ? blocks : (unsigned long long)c->cus * 16ull);
  launch(t4k::kmerExportKernel, grid, 256, c->stream, kc->tb, dC, dV, dCur, (unsigned long long)cap);
  HIPCHK(c, hipGetLastError());
  unsigned long long got = 0;
  HIPCHK(c, hipMemcpyAsync(&got, dCur, sizeof got, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t m = (size_t)(got < (unsigned long long)cap ? got : (unsigned long long)cap);
  if (m) {
    HIPCHK(c, hipMemcpy(codes, dC, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(counts, dV, sizeof(int) * m, hipMemcpyDeviceToHost));
  }
  if (got != used) return fail(c, T4_ERR_STATE, "t4_kmer_count_export: %llu pairs in a table that counted %llu distinct k-mers", got, used);
  return T4_OK;
}

int t4_kmer_count_merge(t4_kmer_counter *kc, const uint64_t *codes, const int32_t *counts, int64_t n, int only_present) {
  if (!kc || n < 0 || (n > 0 && (!codes || !counts))) return T4_ERR_ARG;
  t4_ctx *c = kc->ctx;
  if (n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  int r;
  const int64_t SLICE = (int64_t)1 << 26;   // pairs per upload (768 MB of device memory at most)
  DevBuf<unsigned long long> dC; DevBuf<int> dV;
  const size_t cap = (size_t)(n < SLICE ? n : SLICE);
  if ((r = dC.alloc(c, cap)) || (r = dV.alloc(c, cap))) return r;
  int overflow = 0;
  for (int64_t lo = 0; lo < n && !overflow; lo += SLICE) {
    const int64_t m = n - lo < SLICE ? n - lo : SLICE;
    if (!only_present && (r = kmerEnsureRoom(kc, (unsigned long long)m, true))) return r;
    HIPCHK(c, hipMemcpy(dC, codes + lo, sizeof(unsigned long long) * (size_t)m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dV, counts + lo, sizeof(int) * (size_t)m, hipMemcpyHostToDevice));
    const int grid = (int)((m + 255) / 256 < (long long)c->cus * 8 ? (m + 255) / 256 : (long long)c->cus * 8);
    launch(t4k::kmerMergeKernel, grid, 256, c->stream, kc->tb, (const unsigned long long *)dC, (const int *)dV, (long long)m, only_present ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&overflow, kc->tb.overflow, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (overflow) return fail(c, T4_ERR_UNSUPPORTED, "t4_kmer_count_merge: more distinct k-mers than the table was created for (%llu slots)", kc->slots);
  return T4_OK;
}

namespace {
// kmerStatsKernel over the n > 0 rows of b and its four result arrays to the host; quals / qoff: device pointers, or null for no trimming
int kmerStatsRun(t4_kmer_counter *kc, t4_batch *b, const char *quals, const long long *qoff, int32_t *min_cnt, int32_t *median_cnt, float *avg_cnt, int32_t *new_len) {
  t4_ctx *c = kc->ctx;
  const long long n = b->n;
  int r;
  DevBuf<int> dMin, dMed, dLen; DevBuf<float> dAvg;
  if ((r = dMin.alloc(c, (size_t)n)) || (r = dMed.alloc(c, (size_t)n)) || (r = dLen.alloc(c, (size_t)n)) || (r = dAvg.alloc(c, (size_t)n))) return r;
  const int grid = (int)(n < (long long)c->cus * 32 ? n : (long long)c->cus * 32);
  launch(t4k::kmerStatsKernel, grid, 64, c->stream, b->view, kc->tb, quals, qoff, dMin, dMed, dAvg, dLen);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(min_cnt, dMin, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(median_cnt, dMed, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(avg_cnt, dAvg, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(new_len, dLen, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return T4_OK;
}
}  // namespace

int t4_kmer_count_stats(t4_kmer_counter *kc, t4_batch *b, const char *quals, const int64_t *qual_off,
                        int32_t *min_cnt, int32_t *median_cnt, float *avg_cnt, int32_t *new_len) {
  if (!kc || !b || !min_cnt || !median_cnt || !avg_cnt || !new_len || (quals && !qual_off)) return T4_ERR_ARG;
  t4_ctx *c = kc->ctx;
  if (b->ctx != c) return fail(c, T4_ERR_ARG, "batch belongs to another ctx");
  const long long n = b->n;
  if (n == 0) return T4_OK;
  if (kc->tb.perBarcode && !b->dBarcode) return fail(c, T4_ERR_ARG, "t4_kmer_count_stats: per-barcode counts need a batch uploaded with barcodes");
  if (int fit = kmerBarcodesFit(kc, b, "t4_kmer_count_stats")) return fit;
  (void)hipSetDevice(c->device);
  int r;
  DevBuf<char> dQ; DevBuf<long long> dOff;
  if (quals) {
    std::vector<int> lens((size_t)n);
    HIPCHK(c, hipMemcpy(lens.data(), b->dLen, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    for (long long i = 0; i < n; ++i)
      if (qual_off[i + 1] - qual_off[i] != lens[(size_t)i]) return fail(c, T4_ERR_ARG, "read %lld has %d bases and %lld qualities", i, lens[(size_t)i], (long long)(qual_off[i + 1] - qual_off[i]));
    const size_t qn = (size_t)qual_off[n];
    if ((r = dQ.alloc(c, qn + 16)) || (r = dOff.alloc(c, (size_t)n + 1))) return r;
    if (qn) HIPCHK(c, hipMemcpy(dQ, quals, qn, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dOff, qual_off, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice));
  }
  return kmerStatsRun(kc, b, dQ, dOff, min_cnt, median_cnt, avg_cnt, new_len);
}

int t4_kmer_count_stats_resident(t4_kmer_counter *kc, t4_batch *b, int use_quals, int32_t *min_cnt, int32_t *median_cnt, float *avg_cnt, int32_t *new_len) {
  if (!kc || !b || !min_cnt || !median_cnt || !avg_cnt || !new_len) return T4_ERR_ARG;
  t4_ctx *c = kc->ctx;
  if (b->ctx != c) return fail(c, T4_ERR_ARG, "batch belongs to another ctx");
  if (use_quals && !b->dQoff.p) return fail(c, T4_ERR_ARG, "t4_kmer_count_stats_resident: the batch carries no qualities");
  const long long n = b->n;
  if (n == 0) return T4_OK;
  if (kc->tb.perBarcode && !b->dBarcode) return fail(c, T4_ERR_ARG, "t4_kmer_count_stats_resident: per-barcode counts need a batch uploaded with barcodes");
  if (int fit = kmerBarcodesFit(kc, b, "t4_kmer_count_stats_resident")) return fit;
  (void)hipSetDevice(c->device);
  return kmerStatsRun(kc, b, use_quals ? b->dQual.p : nullptr, use_quals ? b->dQoff.p : nullptr, min_cnt, median_cnt, avg_cnt, new_len);
}

int t4_kmer_count_reserve(t4_kmer_counter *kc, int64_t incoming) {
  if (!kc || incoming < 0) return T4_ERR_ARG;
  (void)hipSetDevice(kc->ctx->device);
  return incoming ? kmerEnsureRoom(kc, (unsigned long long)incoming, true) : T4_OK;
}

int64_t t4_kmer_count_distinct(t4_kmer_counter *kc) {
  if (!kc) return -1;
  t4_ctx *c = kc->ctx;
  (void)hipSetDevice(c->device);
  std::vector<unsigned long long> keys((size_t)kc->slots);
  if (hipMemcpy(keys.data(), kc->tb.keys, sizeof(unsigned long long) * (size_t)kc->slots, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  int64_t d = 0;
  for (unsigned long long x : keys) if (x) ++d;
  return d;
}

int t4_has_hit(t4_index *ref, t4_batch *b, int mode, int32_t *out) {
  if (!ref || !b || !out) return T4_ERR_ARG;
  t4_ctx *c = ref->ctx;
  if (mode != 0) return fail(c, T4_ERR_UNSUPPORTED, "t4_has_hit: only mode 0 (the stage-0 extractor's) is built");
  int r;
  if ((r = ensurePerCall(c, b->n))) return r;
  T4QueryArgs qa;
  memset(&qa, 0, sizeof qa);
  qa.mode = 5; qa.ret = c->counts;
  if ((r = runQuery(ref, b, qa, false))) return r;
  if (b->n > 0) {
    HIPCHK(c, hipMemcpyAsync(out, c->counts, sizeof(int) * (size_t)b->n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return T4_OK;
}

// ---- FASTQ text on the device (t4_text.h) ---------------------------------------------------------------------------------------
int t4_text_create(t4_ctx *c, int64_t max_piece_bytes, t4_text **out) {
  if (!c || !out) return T4_ERR_ARG;
  *out = nullptr;
  // (offsets into a piece are 32-bit words, and nbytes + 1 is one of them)
  if (max_piece_bytes < 1 || max_piece_bytes > ((int64_t)1 << 31)) return fail(c, T4_ERR_ARG, "t4_text_create: a piece has 1 to 2^31 bytes, not %lld", (long long)max_piece_bytes);
  (void)hipSetDevice(c->device);
  std::unique_ptr<t4_text> tx(new t4_text());   // (and its buffers, on every way out but the last)
  tx->ctx = c; tx->cap = max_piece_bytes;
  const size_t tiles = (size_t)((max_piece_bytes + T4_TEXT_TILE - 1) / T4_TEXT_TILE), recs = (size_t)(max_piece_bytes / 4) + 1;
  int r;
  if ((r = tx->stage.alloc(c, (size_t)max_piece_bytes, hipHostMallocDefault)) || (r = tx->infoHost.alloc(c, T4_TEXT_INFO_WORDS, hipHostMallocDefault)) ||
      (r = tx->dText.alloc(c, tiles * T4_TEXT_TILE)) || (r = tx->dTileCnt.alloc(c, tiles)) || (r = tx->dLineStart.alloc(c, (size_t)max_piece_bytes + 2)) ||
      (r = tx->dLen.alloc(c, recs)) || (r = tx->dRecStart.alloc(c, recs)) || (r = tx->dLow.alloc(c, recs)) || (r = tx->dInfo.alloc(c, T4_TEXT_INFO_WORDS)))
    return r;
  *out = tx.release();
  return T4_OK;
}

void t4_text_destroy(t4_text *tx) { delete tx; }

int t4_text_scan(t4_text *tx, const char *text, int64_t nbytes, int final_piece, int64_t info[5]) {
  if (!tx || !info) return T4_ERR_ARG;
  t4_ctx *c = tx->ctx;
  tx->status = -1; tx->nbytes = tx->lines = tx->nrec = tx->recBytes = 0; tx->badRec = -1; tx->longest = 0;
  tx->scanId = ++c->textScans; tx->pairOk = false;
  if (nbytes < 0 || nbytes > tx->cap || (nbytes > 0 && !text)) return fail(c, T4_ERR_ARG, "t4_text_scan: %lld bytes for a handle made for %lld", (long long)nbytes, (long long)tx->cap);
  (void)hipSetDevice(c->device);
  unsigned long long *h = tx->infoHost;
  h[T4_TEXT_NEWLINES] = 0; h[T4_TEXT_BAD] = ~0ull; h[T4_TEXT_LONGEST] = 0; h[T4_TEXT_END] = 0;
  int64_t lines = 0, nrec = 0;
  if (nbytes > 0) {
    const int tiles = (int)((nbytes + T4_TEXT_TILE - 1) / T4_TEXT_TILE);
    const int openEnd = final_piece && text[nbytes - 1] != '\n';
    memcpy(tx->stage, text, (size_t)nbytes);
    HIPCHK(c, hipMemcpyAsync(tx->dText, tx->stage, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tx->dInfo, h, sizeof(unsigned long long) * T4_TEXT_INFO_WORDS, hipMemcpyHostToDevice, c->stream));
    launch(t4k::textCountKernel, tiles, T4_TEXT_THREADS, c->stream, tx->dText, (long long)nbytes, tx->dTileCnt);
    launch(t4k::textScanKernel, 1, T4_TEXT_THREADS, c->stream, tx->dTileCnt, tiles, tx->dInfo);
    launch(t4k::textFillKernel, tiles, T4_TEXT_THREADS, c->stream, tx->dText, (long long)nbytes, tx->dTileCnt, tx->dLineStart, openEnd, tx->dInfo);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, tx->dInfo, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lines = (int64_t)h[T4_TEXT_NEWLINES] + openEnd;
    nrec = lines / 4;
    if (nrec > 0) {
      launch(t4k::textRecordKernel<false>, (int)((nrec * 32 + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS), T4_TEXT_THREADS, c->stream, tx->dText, tx->dLineStart,
             0ll, (long long)nrec, tx->dLen, tx->dLow, tx->dRecStart, tx->dInfo, nullptr, nullptr, 0, 0);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(h, tx->dInfo, sizeof(unsigned long long) * T4_TEXT_INFO_WORDS, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  tx->nbytes = nbytes; tx->lines = lines; tx->nrec = nrec;
  tx->recBytes = nrec ? std::min<int64_t>((int64_t)h[T4_TEXT_END], nbytes) : 0;   // (a last line without '\n' ends at nbytes)
  tx->status = 0;
  if (h[T4_TEXT_BAD] != ~0ull) { tx->status = (int)(h[T4_TEXT_BAD] & 15); tx->badRec = (int64_t)(h[T4_TEXT_BAD] >> 4); }
  else if (final_piece && lines % 4) { tx->status = 8; tx->badRec = nrec; }
  tx->longest = (int)h[T4_TEXT_LONGEST];
  info[0] = nrec; info[1] = tx->recBytes; info[2] = tx->status; info[3] = tx->badRec; info[4] = tx->longest;
  return T4_OK;
}

int t4_text_batch(t4_text *tx, int64_t first, int64_t n, t4_batch **out) {
  if (!tx || !out) return T4_ERR_ARG;
  *out = nullptr;
  t4_ctx *c = tx->ctx;
  if (tx->status < 0) return fail(c, T4_ERR_ARG, "t4_text_batch: no piece has been scanned");
  if (tx->status > 0) return fail(c, T4_ERR_ARG, "t4_text_batch: the piece has status %d at record %lld", tx->status, (long long)tx->badRec);
  if (first < 0 || n < 0 || first + n > tx->nrec) return fail(c, T4_ERR_ARG, "t4_text_batch: records [%lld, %lld) of a piece of %lld", (long long)first, (long long)(first + n), (long long)tx->nrec);
  (void)hipSetDevice(c->device);
  const int grid = (int)((n + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS);
  int maxLen = tx->longest;
  if (n == 0) maxLen = 0;
  else if (n < tx->nrec) {   // a part of the piece: its own longest read, as the host packer would size the rows
    unsigned long long *h = tx->infoHost;
    HIPCHK(c, hipMemsetAsync(tx->dInfo + T4_TEXT_END, 0, sizeof(unsigned long long), c->stream));
    launch(t4k::textMaxLenKernel, grid, T4_TEXT_THREADS, c->stream, tx->dLen + first, (long long)n, tx->dInfo + T4_TEXT_END);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, tx->dInfo + T4_TEXT_END, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    maxLen = (int)h[0];
  }
  std::unique_ptr<t4_batch> b(new t4_batch());
  b->ctx = c; b->n = n; b->maxLen = maxLen;
  b->wpk = std::max(1, (maxLen + 15) / 16); b->wnm = std::max(1, (maxLen + 31) / 32);
  int r;
  if ((r = b->dPk.alloc(c, (size_t)n * b->wpk + 4)) || (r = b->dNm.alloc(c, (size_t)n * b->wnm + 4)) || (r = b->dLen.alloc(c, (size_t)n)) || (r = b->dLow.alloc(c, (size_t)n))) return r;
  if (n > 0) {
    launch(t4k::textRecordKernel<true>, (int)((n * 32 + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS), T4_TEXT_THREADS, c->stream, tx->dText, tx->dLineStart,
           (long long)first, (long long)n, b->dLen, b->dLow, nullptr, nullptr, b->dPk, b->dNm, b->wpk, b->wnm);
    HIPCHK(c, hipGetLastError());
  }
  b->view.pk = b->dPk; b->view.nm = b->dNm; b->view.len = b->dLen; b->view.barcode = nullptr;
  b->view.wpk = b->wpk; b->view.wnm = b->wnm; b->view.n = n;
  *out = b.release();
  return T4_OK;
}

int t4_text_records(t4_text *tx, int64_t first, int64_t n, uint32_t *rec_start, uint8_t *low_complexity) {
  if (!tx) return T4_ERR_ARG;
  t4_ctx *c = tx->ctx;
  if (tx->status < 0) return fail(c, T4_ERR_ARG, "t4_text_records: no piece has been scanned");
  if (first < 0 || n < 0 || first + n > tx->nrec) return fail(c, T4_ERR_ARG, "t4_text_records: records [%lld, %lld) of a piece of %lld", (long long)first, (long long)(first + n), (long long)tx->nrec);
  (void)hipSetDevice(c->device);
  if (rec_start) {
    const int64_t have = std::min<int64_t>(n + 1, tx->nrec - first);   // (record nrec has no entry: it begins where the whole records end)
    if (have > 0) HIPCHK(c, hipMemcpyAsync(rec_start, tx->dRecStart + first, sizeof(uint32_t) * (size_t)have, hipMemcpyDeviceToHost, c->stream));
    if (have < n + 1) rec_start[n] = (uint32_t)tx->recBytes;
  }
  if (low_complexity && n > 0) HIPCHK(c, hipMemcpyAsync(low_complexity, tx->dLow + first, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return T4_OK;
}

int t4_text_process_pairs(t4_text *reads, t4_text *mates, int64_t first_read, int64_t first_mate, int64_t n, const uint8_t *skip,
                          int32_t *meta4, char *out_r, char *out_q, int64_t out_cap, int64_t *out_bytes) {
  if (!reads || !mates || !out_bytes) return T4_ERR_ARG;
  t4_ctx *c = reads->ctx;
  *out_bytes = 0;
  reads->pairOk = false;
  if (mates->ctx != c) return fail(c, T4_ERR_ARG, "t4_text_process_pairs: the two pieces belong to different contexts");
  auto covered = [&]() {   // what t4_text_pairs_batch asks for
    reads->pairOk = true; reads->pairMates = mates; reads->pairFirst[0] = first_read; reads->pairFirst[1] = first_mate; reads->pairN = n;
    reads->pairScan[0] = reads->scanId; reads->pairScan[1] = mates->scanId;
    return T4_OK;
  };
  const t4_text *side[2] = {reads, mates};
  const int64_t firsts[2] = {first_read, first_mate};
  for (int k = 0; k < 2; ++k) {
    const char *what = k ? "mates" : "reads";
    if (side[k]->status < 0) return fail(c, T4_ERR_ARG, "t4_text_process_pairs: no piece of the %s has been scanned", what);
    if (side[k]->status > 0) return fail(c, T4_ERR_ARG, "t4_text_process_pairs: the piece of the %s has status %d at record %lld", what, side[k]->status, (long long)side[k]->badRec);
    if (firsts[k] < 0 || n < 0 || firsts[k] + n > side[k]->nrec)
      return fail(c, T4_ERR_ARG, "t4_text_process_pairs: records [%lld, %lld) of a piece of the %s of %lld", (long long)firsts[k], (long long)(firsts[k] + n), what, (long long)side[k]->nrec);
  }
  if (out_cap < 0 || (n > 0 && !meta4) || (out_cap > 0 && (!out_r || !out_q))) return fail(c, T4_ERR_ARG, "t4_text_process_pairs: no room for the result");
  if (n == 0) return covered();
  (void)hipSetDevice(c->device);
  t4_text *tx = reads;
  int r;
  const size_t recs = (size_t)(tx->cap / 4) + 1;
  if ((!tx->dPairMeta.p && (r = tx->dPairMeta.alloc(c, recs))) || (!tx->dPairSkip.p && (r = tx->dPairSkip.alloc(c, recs))) ||
      (!tx->dPairNeed.p && (r = tx->dPairNeed.alloc(c, 1))) || (!tx->pairNeedHost.p && (r = tx->pairNeedHost.alloc(c, 1, hipHostMallocDefault)))) return r;
  // room on the device: what the caller has, but never more than the changed reads of these two pieces can take (a record spends at
  // least twice its read's length, and offsets are 32-bit words)
  const int64_t room = std::min<int64_t>(std::min<int64_t>(out_cap, (reads->nbytes + mates->nbytes) / 2), 0x7fffffff);
  if (room > tx->pairCap) {
    tx->pairCap = 0;
    if ((r = tx->dPairR.alloc(c, (size_t)room)) || (r = tx->dPairQ.alloc(c, (size_t)room))) return r;
    tx->pairCap = room;
  }
  if (skip) HIPCHK(c, hipMemcpyAsync(tx->dPairSkip, skip, (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(tx->dPairNeed, 0, sizeof(unsigned long long), c->stream));
  const int grid = (int)std::min<int64_t>(n, (int64_t)c->cus * 32);
  launch(t4k::textProcessPairKernel, grid, 64, c->stream, reads->dText, reads->dLineStart, (long long)first_read, mates->dText, mates->dLineStart,
         (long long)first_mate, (long long)n, skip ? tx->dPairSkip.p : nullptr, tx->dPairR, tx->dPairQ, (long long)room, tx->dPairNeed, tx->dPairMeta);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(tx->pairNeedHost, tx->dPairNeed, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(meta4, tx->dPairMeta, sizeof(int4) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t need = (int64_t)tx->pairNeedHost[0];
  *out_bytes = need;
  if (need > room) return fail(c, T4_ERR_ARG, "t4_text_process_pairs: the changed reads take %lld bytes, there is room for %lld", (long long)need, (long long)out_cap);
  if (need > 0) {
    HIPCHK(c, hipMemcpyAsync(out_r, tx->dPairR, (size_t)need, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_q, tx->dPairQ, (size_t)need, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return covered();
}

int t4_text_pairs_batch(t4_text *reads, t4_text *mates, int64_t first_read, int64_t first_mate, int64_t n, int with_quals, t4_batch **out, int64_t info[4]) {
  if (!reads || !mates || !out || !info) return T4_ERR_ARG;
  *out = nullptr;
  info[0] = info[1] = info[2] = info[3] = 0;
  t4_ctx *c = reads->ctx;
  t4_text *tx = reads;
  if (!tx->pairOk || tx->pairMates != mates) return fail(c, T4_ERR_ARG, "t4_text_pairs_batch: the last t4_text_process_pairs call on these two handles did not succeed (or there was none)");
  if (tx->pairScan[0] != reads->scanId || tx->pairScan[1] != mates->scanId) return fail(c, T4_ERR_ARG, "t4_text_pairs_batch: a piece has been scanned again since t4_text_process_pairs");
  if (tx->pairFirst[0] != first_read || tx->pairFirst[1] != first_mate || tx->pairN != n)
    return fail(c, T4_ERR_ARG, "t4_text_pairs_batch: pairs [%lld, %lld) / [%lld, %lld), t4_text_process_pairs covered [%lld, %lld) / [%lld, %lld)", (long long)first_read, (long long)(first_read + n),
                (long long)first_mate, (long long)(first_mate + n), (long long)tx->pairFirst[0], (long long)(tx->pairFirst[0] + tx->pairN), (long long)tx->pairFirst[1], (long long)(tx->pairFirst[1] + tx->pairN));
  (void)hipSetDevice(c->device);
  int r;
  long long rows = 0, bases = 0;
  int longest = 0;
  unsigned long long *h = nullptr;
  const size_t recs = (size_t)(tx->cap / 4) + 1, maxBlocks = (recs + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS;   // workgroups of the row scan: rows, then bases in dRowBlock
  if (n > 0) {
    if ((!tx->dRowAt.p && (r = tx->dRowAt.alloc(c, recs))) || (!tx->dRowBlock.p && (r = tx->dRowBlock.alloc(c, 2 * maxBlocks))) ||
        (!tx->dRowInfo.p && (r = tx->dRowInfo.alloc(c, T4_PAIRROWS_WORDS))) || (!tx->rowInfoHost.p && (r = tx->rowInfoHost.alloc(c, T4_PAIRROWS_WORDS, hipHostMallocDefault)))) return r;
    h = tx->rowInfoHost;
    const int blocks = (int)((n + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS);
    HIPCHK(c, hipMemsetAsync(tx->dRowInfo, 0, sizeof(unsigned long long) * T4_PAIRROWS_WORDS, c->stream));
    launch(t4k::textPairRowsKernel, blocks, T4_TEXT_THREADS, c->stream, tx->dPairMeta, mates->dLineStart, (long long)first_mate, (long long)n, tx->dRowAt,
           tx->dRowBlock, tx->dRowBlock + maxBlocks, tx->dRowInfo);
    launch(t4k::textPairScanKernel, 1, T4_TEXT_THREADS, c->stream, tx->dRowBlock, tx->dRowBlock + maxBlocks, blocks, tx->dRowInfo);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, tx->dRowInfo, sizeof(unsigned long long) * T4_PAIRROWS_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rows = (long long)h[T4_PAIRROWS_ROWS]; bases = (long long)h[T4_PAIRROWS_BASES]; longest = (int)h[T4_PAIRROWS_LONGEST];
    info[0] = rows; info[1] = bases; info[2] = longest;
    if (longest > T4_MAXL) return fail(c, T4_ERR_UNSUPPORTED, "t4_text_pairs_batch: a read of %d bases (a merged read may reach the length of both mates), a batch takes %d", longest, T4_MAXL);
  }
  std::unique_ptr<t4_batch> b(new t4_batch());
  b->ctx = c; b->n = rows; b->maxLen = longest;
  b->wpk = std::max(1, (longest + 15) / 16); b->wnm = std::max(1, (longest + 31) / 32);
  if ((r = b->dPk.alloc(c, (size_t)rows * b->wpk + 4)) || (r = b->dNm.alloc(c, (size_t)rows * b->wnm + 4)) || (r = b->dLen.alloc(c, (size_t)rows)) || (r = b->dLow.alloc(c, (size_t)rows))) return r;
  if (with_quals) {
    if ((r = b->dQual.alloc(c, (size_t)bases + 16)) || (r = b->dQoff.alloc(c, (size_t)rows + 1))) return r;
    b->qualBytes = bases;
    if (rows == 0) HIPCHK(c, hipMemsetAsync(b->dQoff, 0, sizeof(long long), c->stream));
  }
  if (rows > 0) {
    HIPCHK(c, hipMemsetAsync(b->dLow, 0, (size_t)rows, c->stream));
    launch(t4k::textPairPackKernel, (int)((n * 32 + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS), T4_TEXT_THREADS, c->stream, reads->dText, reads->dLineStart, (long long)first_read,
           mates->dText, mates->dLineStart, (long long)first_mate, (long long)n, tx->dPairMeta, tx->dPairR, tx->dPairQ, (long long)tx->pairCap, tx->dRowAt, tx->dRowBlock,
           tx->dRowBlock + maxBlocks, b->dPk, b->dNm, b->wpk, b->wnm, b->dLen, b->dQual, b->dQoff, tx->dRowInfo);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h + T4_PAIRROWS_OTHER, tx->dRowInfo + T4_PAIRROWS_OTHER, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    info[3] = h[T4_PAIRROWS_OTHER] ? 1 : 0;
  }
  b->view.pk = b->dPk; b->view.nm = b->dNm; b->view.len = b->dLen; b->view.barcode = nullptr;
  b->view.wpk = b->wpk; b->view.wnm = b->wnm; b->view.n = rows;
  *out = b.release();
  return T4_OK;
}

// (tests) the line table of the piece last scanned: lines + 1 offsets
int t4_text_lines(t4_text *tx, uint32_t *line_start, int64_t cap, int64_t *lines) {
  if (!tx || !lines || tx->status < 0) return T4_ERR_ARG;
  t4_ctx *c = tx->ctx;
  *lines = tx->lines;
  if (!line_start || tx->nbytes == 0) return T4_OK;   // (an empty piece has no table)
  if (cap < tx->lines + 1) return fail(c, T4_ERR_ARG, "t4_text_lines: room for %lld offsets, the piece has %lld", (long long)cap, (long long)tx->lines + 1);
  HIPCHK(c, hipMemcpy(line_start, tx->dLineStart, sizeof(uint32_t) * (size_t)(tx->lines + 1), hipMemcpyDeviceToHost));
  return T4_OK;
}
int t4_text_tile_bytes(void) { return T4_TEXT_TILE; }

// (tests) the rows of a batch: dims = words per pk row, words per nm row, longest read; low: zeros for a batch without such bytes
int t4_batch_read(t4_batch *b, int32_t dims[3], uint32_t *pk, uint32_t *nm, int32_t *len, uint8_t *low) {
  if (!b) return T4_ERR_ARG;
  t4_ctx *c = b->ctx;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (dims) { dims[0] = b->wpk; dims[1] = b->wnm; dims[2] = b->maxLen; }
  const size_t n = (size_t)b->n;
  if (n == 0) return T4_OK;
  if (pk) HIPCHK(c, hipMemcpy(pk, b->dPk, sizeof(uint32_t) * n * b->wpk, hipMemcpyDeviceToHost));
  if (nm) HIPCHK(c, hipMemcpy(nm, b->dNm, sizeof(uint32_t) * n * b->wnm, hipMemcpyDeviceToHost));
  if (len) HIPCHK(c, hipMemcpy(len, b->dLen, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (low) { if (b->dLow.p) HIPCHK(c, hipMemcpy(low, b->dLow, n, hipMemcpyDeviceToHost)); else memset(low, 0, n); }
  return T4_OK;
}

// (tests) the qualities a batch carries: *nbytes = how many (-1: none, nothing else is written), quals (room for cap >= *nbytes, or null), qual_off (n + 1 offsets, or null)
int t4_batch_quals(t4_batch *b, char *quals, int64_t cap, int64_t *qual_off, int64_t *nbytes) {
  if (!b || !nbytes) return T4_ERR_ARG;
  t4_ctx *c = b->ctx;
  *nbytes = b->dQoff.p ? (int64_t)b->qualBytes : -1;
  if (!b->dQoff.p) return T4_OK;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (quals && cap < b->qualBytes) return fail(c, T4_ERR_ARG, "t4_batch_quals: room for %lld bytes, the batch has %lld", (long long)cap, b->qualBytes);
  if (quals && b->qualBytes > 0) HIPCHK(c, hipMemcpy(quals, b->dQual, (size_t)b->qualBytes, hipMemcpyDeviceToHost));
  if (qual_off) HIPCHK(c, hipMemcpy(qual_off, b->dQoff, sizeof(long long) * ((size_t)b->n + 1), hipMemcpyDeviceToHost));
  return T4_OK;
}

int t4_candidate_test(t4_index *ref, t4_batch *reads, t4_batch *mates, uint8_t *keep) {
  if (!ref || !reads || !keep) return T4_ERR_ARG;
  t4_ctx *c = ref->ctx;
  if (mates && mates->n != reads->n) return fail(c, T4_ERR_ARG, "t4_candidate_test: %lld reads and %lld mates", reads->n, mates->n);
  if (reads->ctx != c || (mates && mates->ctx != c)) return fail(c, T4_ERR_ARG, "batch belongs to another ctx");
  const long long n = reads->n;
  if (n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  DevBuf<int> qlen;
  DevBuf<unsigned char> pass1, pass;
  int r;
  if ((r = qlen.alloc(c, (size_t)n)) || (r = pass1.alloc(c, (size_t)n)) || (mates && (r = pass.alloc(c, (size_t)n)))) return r;
  const int grid = (int)((n + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS);
  // one side: the rows that are still to be tested keep their length, the others are queried as empty reads (HasHitInSet = 0)
  auto side = [&](t4_batch *b, const unsigned char *done, unsigned char *out) -> int {
    int rr;
    if ((rr = ensurePerCall(c, n))) return rr;
    launch(t4k::candLenKernel, grid, T4_TEXT_THREADS, c->stream, b->dLen, b->dLow, done, qlen, n);
    HIPCHK(c, hipGetLastError());
    T4QueryArgs qa;
    memset(&qa, 0, sizeof qa);
    qa.mode = 5; qa.ret = c->counts;
    b->view.len = qlen;
    rr = runQuery(ref, b, qa, false);
    b->view.len = b->dLen;
    if (rr) return rr;
    launch(t4k::candCombineKernel, grid, T4_TEXT_THREADS, c->stream, qlen, c->counts, done, out, n);
    HIPCHK(c, hipGetLastError());
    return T4_OK;
  };
  if ((r = side(reads, nullptr, pass1))) return r;
  if (mates && (r = side(mates, pass1, pass))) return r;
  HIPCHK(c, hipMemcpyAsync(keep, mates ? pass.p : pass1.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return T4_OK;
}

int t4_assign(t4_index *ix, t4_batch *b, int strand, int32_t *ret, t4_overlap *out) {
  if (!ix || !b) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (ix->committed && ix->view.firstIsRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_assign needs a contig set (ExtendOverlap aligns against posWeight)");
  int r;
  if ((r = ensurePerCall(c, b->n))) return r;
  if ((r = ensureResult(c, (size_t)b->n))) return r;
  T4QueryArgs qa;
  memset(&qa, 0, sizeof qa);
  qa.mode = 2; qa.strand = strand; qa.skipRepeats = 0; qa.maxPerRead = 1; qa.counts = nullptr; qa.out = c->result; qa.ret = c->counts;
  if ((r = runQuery(ix, b, qa, true))) return r;
  if (ret && b->n) HIPCHK(c, hipMemcpy(ret, c->counts, sizeof(int) * (size_t)b->n, hipMemcpyDeviceToHost));
  if (out && b->n) HIPCHK(c, hipMemcpy(out, c->result, sizeof(t4_overlap) * (size_t)b->n, hipMemcpyDeviceToHost));
  return T4_OK;
}

int t4_assign_strands(t4_index *ix, t4_batch *b, const int32_t *strands, int32_t *ret, t4_overlap *out) {
  if (!ix || !b || (b->n > 0 && !strands)) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (ix->committed && ix->view.firstIsRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_assign_strands needs a contig set (ExtendOverlap aligns against posWeight)");
  if (b->n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  int r;
  if ((r = ensurePerCall(c, b->n))) return r;
  if ((r = ensureResult(c, (size_t)b->n))) return r;
  DevBuf<int> dSt;
  if ((r = dSt.alloc(c, (size_t)b->n))) return r;
  HIPCHK(c, hipMemcpy(dSt, strands, sizeof(int) * (size_t)b->n, hipMemcpyHostToDevice));
  T4QueryArgs qa;
  memset(&qa, 0, sizeof qa);
  qa.mode = 2; qa.strand = 0; qa.strandPerRead = dSt; qa.skipRepeats = 0; qa.maxPerRead = 1; qa.counts = nullptr; qa.out = c->result; qa.ret = c->counts;
  if ((r = runQuery(ix, b, qa, true))) return r;
  if (ret) HIPCHK(c, hipMemcpy(ret, c->counts, sizeof(int) * (size_t)b->n, hipMemcpyDeviceToHost));
  if (out) HIPCHK(c, hipMemcpy(out, c->result, sizeof(t4_overlap) * (size_t)b->n, hipMemcpyDeviceToHost));
  return T4_OK;
}

}  // extern "C"

namespace {
int assignWidePass2(t4_index *ix, t4_batch *b, const std::vector<int64_t> &todo, int strand, const int32_t *strands, int32_t *ret, t4_overlap *out);
const int ASSIGN_WIDE_BATCH = 256;   // reads of one AddRead query call of pass 2 (its first launch gives every read a workgroup with a slice of global scratch)
}  // namespace

extern "C" {

int t4_assign_wide(t4_index *ix, t4_batch *b, int strand, const int32_t *strands, int32_t *ret, t4_overlap *out) {
  if (!ix || !b) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  c->assignWide[0] = c->assignWide[1] = 0;
  if (ix->committed && ix->view.firstIsRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_assign_wide needs a contig set (ExtendOverlap aligns against posWeight)");
  if (!ix->committed) return fail(c, T4_ERR_STATE, "index not committed");
  if (b->ctx != c) return fail(c, T4_ERR_ARG, "batch belongs to another ctx");
  if (c->aq.active) return fail(c, T4_ERR_STATE, "an AddRead query is already in flight on this ctx");
  if (b->n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)b->n;
  std::vector<int64_t> todo;   // the reads of pass 2
  if (getenv("T4_ASSIGN_WIDE_ALL")) {   // testing aid, read once per call: every read takes the wide route (and none the tiers)
    todo.resize(n);
    for (size_t i = 0; i < n; ++i) todo[i] = (int64_t)i;
  } else {
    // pass 1: t4_assign / t4_assign_strands, with the reads beyond the tiers' limits reported instead of refused
    int r;
    if ((r = ensurePerCall(c, b->n))) return r;
    if ((r = ensureResult(c, n))) return r;
    DevBuf<int> dSt;
    if (strands) {
      if ((r = dSt.alloc(c, n))) return r;
      HIPCHK(c, hipMemcpy(dSt, strands, sizeof(int) * n, hipMemcpyHostToDevice));
    }
    T4QueryArgs qa;
    memset(&qa, 0, sizeof qa);
    qa.mode = 2; qa.strand = strands ? 0 : strand; qa.strandPerRead = strands ? (const int *)dSt : nullptr; qa.skipRepeats = 0; qa.maxPerRead = 1;
    qa.counts = nullptr; qa.out = c->result; qa.ret = c->counts;
    std::vector<int> status;
    if ((r = runQuery(ix, b, qa, true, false, &status))) return r;
    if (ret) HIPCHK(c, hipMemcpy(ret, c->counts, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (out) HIPCHK(c, hipMemcpy(out, c->result, sizeof(t4_overlap) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) if (status[i] != 0) todo.push_back((int64_t)i);
  }
  c->assignWide[0] = (int64_t)(n - todo.size()); c->assignWide[1] = (int64_t)todo.size();
  if (todo.empty()) return T4_OK;
  return assignWidePass2(ix, b, todo, strand, strands, ret, out);
}

int t4_assign_wide_stats(t4_ctx *c, int64_t *out2) {
  if (!c || !out2) return T4_ERR_ARG;
  out2[0] = c->assignWide[0]; out2[1] = c->assignWide[1];
  return T4_OK;
}

int t4_posweight_recompute(t4_index *ix, t4_batch *b, const t4_overlap *assign, const int32_t *mult, int32_t *posweight, int64_t posweight_cap) {
  return t4_consensus_recompute(ix, b, assign, mult, posweight, posweight_cap, nullptr, 0, nullptr);
}

int t4_consensus_recompute(t4_index *ix, t4_batch *b, const t4_overlap *assign, const int32_t *mult, int32_t *posweight, int64_t posweight_cap,
                           char *consensus, int64_t consensus_cap, int64_t *changed) {
  if (!ix || !b || (b->n > 0 && !assign) || !posweight) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (!ix->committed) return fail(c, T4_ERR_STATE, "index not committed");
  if (ix->live) return fail(c, T4_ERR_UNSUPPORTED, "t4_posweight_recompute takes a committed contig set (the extendedSeq of main.cpp:2047), not a live one");
  if (b->ctx != c) return fail(c, T4_ERR_ARG, "batch belongs to another ctx");
  int64_t bases = 0;
  for (const HostSeq &q : ix->seqs) { if (q.isRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_posweight_recompute needs a contig set"); bases += (int64_t)q.cons.size(); }
  if (posweight_cap < 4 * bases) return fail(c, T4_ERR_ARG, "posweight buffer holds %lld values, the set needs %lld", (long long)posweight_cap, (long long)(4 * bases));
  if (consensus && consensus_cap < bases) return fail(c, T4_ERR_ARG, "consensus buffer holds %lld bases, the set has %lld", (long long)consensus_cap, (long long)bases);
  if (changed) *changed = 0;
  if (bases == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  int r;
  DevBuf<int> dCnt, dMult;
  DevBuf<T4OverlapOut> dAs;
  DevBuf<char> dCons;
  DevBuf<unsigned long long> dChanged;
  const size_t n = (size_t)b->n;
  const size_t cols = (size_t)bases + ix->seqs.size();   // the image's column space: every contig is followed by one terminator column (T4SeqInfo::pwOff)
  if ((r = dCnt.alloc(c, cols * 4))) return r;
  HIPCHK(c, hipMemsetAsync(dCnt, 0, sizeof(int) * cols * 4, c->stream));   // posWeight.SetZero of every contig
  if (n > 0) {
    if ((r = dAs.alloc(c, n))) return r;
    HIPCHK(c, hipMemcpyAsync(dAs, assign, sizeof(t4_overlap) * n, hipMemcpyHostToDevice, c->stream));
    if (mult) {
      if ((r = dMult.alloc(c, n))) return r;
      HIPCHK(c, hipMemcpyAsync(dMult, mult, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    }
    const int grid = (int)(n < (size_t)c->cus * 32 ? n : (size_t)c->cus * 32);
    launch(t4k::posWeightAccumulateKernel, grid, 64, c->stream, ix->view, b->view, (const T4OverlapOut *)dAs, (const int *)dMult, dCnt);
    HIPCHK(c, hipGetLastError());
  }
  {
    const int nseq = (int)ix->seqs.size();
    const int grid = nseq < c->cus * 8 ? nseq : c->cus * 8;
    launch(t4k::posWeightFinishKernel, grid > 0 ? grid : 1, 256, c->stream, ix->view, dCnt);
    HIPCHK(c, hipGetLastError());
  }
  std::vector<char> allCons;
  unsigned long long nChanged = 0;
  if (consensus) {   // UpdateConsensus of every contig from the columns just rebuilt
    if ((r = dCons.alloc(c, cols))) return r;
    if ((r = dChanged.alloc(c, 1))) return r;
    HIPCHK(c, hipMemsetAsync(dChanged, 0, sizeof(unsigned long long), c->stream));
    const int nseq = (int)ix->seqs.size();
    const int grid = nseq < c->cus * 8 ? nseq : c->cus * 8;
    launch(t4k::consensusArgmaxKernel, grid > 0 ? grid : 1, 256, c->stream, ix->view, (const int *)dCnt, dCons, dChanged);
    HIPCHK(c, hipGetLastError());
    allCons.resize(cols);
    HIPCHK(c, hipMemcpyAsync(allCons.data(), dCons, cols, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&nChanged, dChanged, sizeof nChanged, hipMemcpyDeviceToHost, c->stream));
  }
  std::vector<int32_t> all(cols * 4);
  HIPCHK(c, hipMemcpyAsync(all.data(), dCnt, sizeof(int) * cols * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (changed) *changed = (int64_t)nChanged;
  {   // contig after contig, without the terminator columns
    size_t from = 0, to = 0;
    for (const HostSeq &q : ix->seqs) {
      const size_t ln = q.cons.size();
      if (ln) memcpy(posweight + 4 * to, all.data() + 4 * from, sizeof(int32_t) * 4 * ln);
      if (ln && consensus) memcpy(consensus + to, allCons.data() + from, ln);
      from += ln + 1; to += ln;
    }
  }
  return T4_OK;
}

int t4_extend(t4_index *ix, t4_batch *b, int max_per_read, const int32_t *counts, const t4_overlap *in, double mismatch_factor,
              int32_t *ret, t4_overlap *out) {
  if (!ix || !b || max_per_read <= 0 || (b->n > 0 && (!counts || !in))) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (ix->committed && ix->view.firstIsRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_extend needs a contig set (ExtendOverlap aligns against posWeight)");
  if (max_per_read > 128) return fail(c, T4_ERR_UNSUPPORTED, "t4_extend takes at most 128 overlaps per read");
  const size_t n = (size_t)b->n, m = n * max_per_read;
  if (n == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  int r;
  if ((r = ensurePerCall(c, b->n))) return r;
  if ((r = ensureResult(c, m))) return r;
  DevBuf<T4OverlapOut> dIn;
  DevBuf<int> dCnt, dRet;
  if ((r = dIn.alloc(c, m)) || (r = dCnt.alloc(c, n)) || (r = dRet.alloc(c, m))) return r;
  HIPCHK(c, hipMemcpy(dIn, in, sizeof(t4_overlap) * m, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dCnt, counts, sizeof(int) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemset(dRet, 0, sizeof(int) * m));
  T4QueryArgs qa;
  memset(&qa, 0, sizeof qa);
  qa.mode = 3; qa.maxPerRead = max_per_read; qa.out = c->result; qa.in = dIn; qa.inCounts = dCnt; qa.ret = dRet; qa.mismatchFactor = mismatch_factor;
  if ((r = runQuery(ix, b, qa, true, true))) return r;
  if (ret) HIPCHK(c, hipMemcpy(ret, dRet, sizeof(int) * m, hipMemcpyDeviceToHost));
  if (out) HIPCHK(c, hipMemcpy(out, c->result, sizeof(t4_overlap) * m, hipMemcpyDeviceToHost));
  return T4_OK;
}

}  // extern "C"

namespace {
// The query half of SeqSet::AddRead for a batch of reads, lean path: one blob in, a small header blob out, and the result
// records written by the kernel straight into a pinned host pool (variable number per read, SeqSet's std::vector<_overlap>):
// one launch (plus one per overflow tier that is needed) and one stream synchronisation per call. Either every read is
// matched against `base` (viewOf == nullptr; first launch on the 8192-hit LDS tier) or read i against views[viewOf[i]]
// (per-barcode images: reads meet a handful of contigs, so the first launch is the 1024-hit tier at 6 groups / CU).
// On return counts[i] records of read i start at index base[i] of ov / ext / ret (valid until the next call on this ctx).
struct AqResult { const int32_t *counts, *base; const t4_overlap *ov, *ext; const int32_t *ret; };
double secondsSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
// tierHint (nullable, in/out): nonzero = the read is known to outgrow the LDS tiers, it is launched on the global-scratch tier
// at once, on a second stream beside the LDS tier; on return nonzero for every read the global-scratch tier served.
int aqLaunch(t4_ctx *c);
// a blob's device copy and its pinned, mapped twin on the host: room for twice what the call needs when they have to grow
int growBlob(t4_ctx *c, size_t need, size_t *cap, DevBuf<unsigned char> &dev, PinnedBuf<unsigned char> &host) {
  if (need <= *cap) return T4_OK;
  *cap = 0;
  int r;
  if ((r = dev.alloc(c, need * 2)) || (r = host.alloc(c, need * 2, hipHostMallocMapped))) return r;
  *cap = need * 2;
  return T4_OK;
}
int aqBegin(t4_ctx *c, const T4IndexView &base, const T4IndexView *views, const int32_t *viewOf, bool smallFirst, int n, const char *bases,
            const int64_t *offsets, const int32_t *barcodes, const int32_t *strands, int skip_repeats, const double *factors,
            unsigned char *tierHint = nullptr, bool lean = false, const int32_t *onlySeq = nullptr, const int32_t *forceMin = nullptr, int wantCands = 0) {
  // (wantCands: bit 0 the candidate store, bit 1 T4CandArgs::extAux)
  (void)hipSetDevice(c->device);
  AqCall &q = c->aq;
  if (q.active) return fail(c, T4_ERR_STATE, "an AddRead query is already in flight on this ctx");
  int maxLen = 1;
  for (int i = 0; i < n; ++i) {
    int64_t l = offsets[i + 1] - offsets[i];
    if (l < 0 || l > T4_MAXL) return fail(c, T4_ERR_UNSUPPORTED, "read %d is %lld bp; this engine takes reads up to %d bp", i, (long long)l, T4_MAXL);
    if (l > maxLen) maxLen = (int)l;
  }
  q.lean = lean;
  q.base = base; q.views = views; q.hasViewOf = viewOf != nullptr; q.smallFirst = smallFirst; q.n = n; q.skipRepeats = skip_repeats; q.tierHint = tierHint; q.attempt = 0;
  const int wpk = (maxLen + 15) / 16, wnm = (maxLen + 31) / 32;
  q.wpk = wpk; q.wnm = wnm;
  // (armed restricted re-queries of reads with long lists: two words per read and the head bitmaps; nothing without them)
  q.hasArm = false;
  if (!c->armWords.empty()) {
    if (!onlySeq || c->armWords.size() != 2 * (size_t)n) { c->armWords.clear(); c->armHead.clear(); return fail(c, T4_ERR_ARG, "t4_add_query_arm_long_lists armed %d reads; the call that follows has %d%s", (int)(c->armWords.size() / 2), n, onlySeq ? "" : " and no restricted re-query"); }
    q.hasArm = true;
  }
  q.hasOnly = onlySeq != nullptr; q.hasForce = forceMin != nullptr; q.wantCands = (wantCands & 1) != 0; q.keepExtAux = (wantCands & 2) != 0;
  const size_t N = (size_t)n, nW = N * (skip_repeats ? 2 : 1);   // (a first pass that finds nothing leaves its slot and takes a new one in the second sweep)
  q.nWideSlots = (int)nW;
  // the two blobs, field by field in the order they lie in memory (a field that does not apply to the call has no elements)
  AqInput &in = q.in;
  in.header = false; in.bytes = 0;
  in.add(in.pk, N * wpk); in.add(in.nm, N * wnm); in.add(in.len, N); in.add(in.barcode, N); in.add(in.strand, N); in.add(in.list, N); in.add(in.viewOf, N); in.add(in.factor, N);
  in.add(in.onlySeq, N); in.add(in.forceMin, N); in.add(in.arm, q.hasArm ? 2 * N : 0); in.add(in.head, q.hasArm ? c->armHead.size() : 0);
  in.add(in.cs, 1); in.add(in.wide[0], 1); in.add(in.wide[1], 1);
  AqHeader &hdr = q.hdr;
  hdr.header = true; hdr.bytes = 0;
  hdr.add(hdr.counts, N); hdr.add(hdr.status, N); hdr.add(hdr.next, N); hdr.add(hdr.next2, N); hdr.add(hdr.outBase, N); hdr.add(hdr.ticks, N); hdr.add(hdr.stable, N);
  hdr.add(hdr.aux, N); hdr.add(hdr.n4, N); hdr.add(hdr.candBase, N); hdr.add(hdr.candCnt, N); hdr.add(hdr.stats8, T4_QSTATS * N); hdr.add(hdr.rorInfo, q.hasArm ? N : 0);
  hdr.add(hdr.tail, 1);
  for (auto &h : hdr.wide) { hdr.add(h.ctl, T4_WC_WORDS); hdr.add(h.plan, nW); hdr.add(h.stat, T4_WIDE_STAT * nW); }
  q.wideSafety = c->wideSafetyKeep;
  int r;
  if ((r = growBlob(c, in.bytes, &c->aqInBytes, c->aqIn, c->aqInHost)) || (r = growBlob(c, hdr.bytes, &c->aqOutBytes, c->aqOut, c->aqOutHost))) return r;
  const auto tp0 = std::chrono::steady_clock::now();
  memset(c->aqInHost, 0, q.in.bytes);
  if (q.hasArm) {   // (consumed: the arming holds for this call alone)
    std::copy(c->armWords.begin(), c->armWords.end(), q.in.arm.stage(c));
    std::copy(c->armHead.begin(), c->armHead.end(), q.in.head.stage(c));
    c->armWords.clear(); c->armHead.clear();
  }
  unsigned *pk = q.in.pk.stage(c), *nm = q.in.nm.stage(c);
  int *len = q.in.len.stage(c), *bc = q.in.barcode.stage(c), *st = q.in.strand.stage(c), *ls = q.in.list.stage(c), *vw = q.in.viewOf.stage(c);
  int *only = q.in.onlySeq.stage(c), *force = q.in.forceMin.stage(c);
  double *fa = q.in.factor.stage(c);
  for (int i = 0; i < n; ++i) {
    const char *s = bases + offsets[i];
    int l = (int)(offsets[i + 1] - offsets[i]);
    len[i] = l; bc[i] = barcodes ? barcodes[i] : -1; st[i] = strands[i]; fa[i] = factors[i]; vw[i] = viewOf ? viewOf[i] : 0;
    only[i] = onlySeq ? onlySeq[i] : -1;
    force[i] = forceMin ? forceMin[i] : 0;
    unsigned *p = pk + (size_t)i * wpk, *qn = nm + (size_t)i * wnm;
    for (int j = 0; j < l; ++j) {
      int v = nucNum(s[j]);
      if (v < 0) {
        if (s[j] != 'N') return fail(c, T4_ERR_UNSUPPORTED, "read %d has base '%c' (alphabet is ACGTN)", i, s[j]);
        qn[j >> 5] |= 1u << (j & 31); v = 0;
      }
      p[j >> 4] |= (unsigned)v << ((j & 15) * 2);
    }
  }
  // one big contig set, plain passes: a read beyond the LDS tier goes to the wide query (t4_wide.h) instead of one workgroup's
  // global scratch -- decided on the device, inside the one launch every read starts in (T4_WIDE_OFF: the global-scratch tier as before)
  // (skipRepeats queries -- --trimLevel 2 -- and barcoded reads on an index that is not keyed by barcode are deferred too: wideWant in processRead)
  q.wide = !views && !smallFirst && base.hasNovel == 2 && !getenv("T4_WIDE_OFF");   // (read per call: tests/test_wide_query.py switches it between two calls on one ctx)
  q.onlyRestricted = false;
  if (onlySeq) {   // a round of restricted re-queries only defers nothing: the wide query's five grids stay unlaunched, and its reads
    bool anyWhole = false;   // (a few overlaps with one contig each) extend inside the query kernel -- no extendKernel behind it
    for (int i = 0; i < n && !anyWhole; ++i) anyWhole = onlySeq[i] < 0;
    if (!anyWhole) { q.wide = false; q.onlyRestricted = !views && !smallFirst; }
  }
  // work lists: the reads of the first LDS launch, then those that go to the global-scratch tier at once
  const bool forceGlobal = c->aqEnv.forceGlobal;   // testing aid: every read on the global-scratch tier
  if (forceGlobal && !smallFirst) { q.allGlobal.assign((size_t)n, 1); q.tierHint = tierHint = q.allGlobal.data(); q.wide = false; }
  // (with the wide query on, a hinted read -- served wide the last time -- starts on the second stream: wideSeedKernel)
  // (not a barcoded read on an index keyed by barcode: those stay with one workgroup)
  auto direct = [&](int i) { return tierHint && tierHint[i] && !smallFirst && !(onlySeq && onlySeq[i] >= 0) && !(q.wide && base.considerBarcode && barcodes && barcodes[i] != -1); };
  int nFirst = 0, nDirect = 0;
  for (int i = 0; i < n; ++i) if (!direct(i)) ls[nFirst++] = i;
  for (int i = 0; i < n; ++i) if (direct(i)) ls[nFirst + nDirect++] = i;
  q.nFirst = nFirst; q.nDirect = nDirect;
  c->aqSecPack += secondsSince(tp0);
  r = aqLaunch(c);
  if (r == T4_OK) q.active = true;
  return r;
}

// The five kernels of the wide query behind its seed stage, on `stream`. The grids are persistent (any size serves any number of
// reads / partitions; an empty grid of several hundred 100 KB-LDS workgroups still takes microseconds to come and go): the caller
// sizes them by what it knows of the reads (wideGrid*), wk is the work description the chain and merge kernels score with.
int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
int wideCus(const t4_ctx *c) { return c->cus > 0 ? c->cus : 1; }
int wideGridParts(const t4_ctx *c, int want) { return clampi(want, 4, wideCus(c) * 2); }
int wideGridReads(const t4_ctx *c, int want) { return clampi(want, 1, wideCus(c) < 64 ? wideCus(c) : 64); }
void launchWideSeed(t4_ctx *c, hipStream_t stream, const T4Wide &w, const T4Work &wk, const int *list, int nList, int firstPass) {   // the seed stage of the reads `list` (device)
  const AqCall &q = c->aq;
  hipLaunchKernelGGL(t4k::wideSeedKernel, dim3(nList < wideCus(c) ? nList : wideCus(c)), dim3(512), 0, stream, q.base, q.bv, wk, q.qa, w, list, nList, firstPass);
}
void launchWide(t4_ctx *c, hipStream_t stream, const T4Wide &w, const T4Work &wk, int gParts, int gReads) {
  const AqCall &q = c->aq;
  const int cus = wideCus(c);
  hipLaunchKernelGGL(t4k::wideScatterKernel, dim3(clampi(8 * gParts, 16, cus * 8)), dim3(256), 0, stream, q.base, w);   // (a partition is planned for four of the kernel's chunks)
  hipLaunchKernelGGL((t4k::wideSortKernel<8192>), dim3(gParts), dim3(512), 0, stream, q.base, w);
  hipLaunchKernelGGL(t4k::wideStatsKernel, dim3(gReads), dim3(512), 0, stream, q.base, w);
  hipLaunchKernelGGL((t4k::wideChainKernel<8192, 1 << T4_WIDE_OVBITS>), dim3(gParts < cus ? gParts : cus), dim3(512), 0, stream, q.base, q.bv, wk, q.qa, w);
  hipLaunchKernelGGL(t4k::wideMergeKernel, dim3(gReads), dim3(512), 0, stream, q.base, q.bv, wk, q.qa, w);
}
// extendKernel over the records of the result pool from `firstRec` on, spread over the chip
int launchExtend(t4_ctx *c, int firstRec) {
  const AqCall &q = c->aq;
  hipLaunchKernelGGL(t4k::extendKernel, dim3(c->cus * 16), dim3(64), 0, c->stream, q.base, q.bv, q.qa, firstRec < c->aqPoolCap ? firstRec : c->aqPoolCap);
  HIPCHK(c, hipGetLastError());
  return T4_OK;
}
int aqLaunchEpilogue(t4_ctx *c) {   // the header block into pinned host memory, then the call's sequence number into the word the host polls (aqEpilogueKernel)
  AqCall &q = c->aq;
  const unsigned long long outW = q.hdr.bytes >> 3;
  const int grid = clampi((int)((outW + 4095) / 4096), 1, 64);
  ++c->aqSeq;
  if (c->aqSeq == 0) c->aqSeq = 1;
  hipLaunchKernelGGL(t4k::aqEpilogueKernel, dim3(grid), dim3(256), 0, c->stream, (const unsigned long long *)c->aqOut.p, (unsigned long long *)c->aqOutHost.dev, outW,
                     c->aqDoneCtr.p, c->aqFlag.dev, c->aqSeq);
  HIPCHK(c, hipGetLastError());
  return T4_OK;
}

// copies, kernels and the header copy of one attempt, enqueued on the ctx's stream (nothing waits here)
int aqLaunch(t4_ctx *c) {
  AqCall &q = c->aq;
  const int n = q.n, nFirst = q.nFirst, nDirect = q.nDirect;
  const bool smallFirst = q.smallFirst;
  int r;
  if (!c->aqPool) {
    if (!c->aqPoolCap) c->aqPoolCap = c->aqEnv.poolCap > 0 ? c->aqEnv.poolCap : 1 << 16;   // (testing aid: a small pool forces the grow-and-repeat path)
    if ((r = c->aqPool.alloc(c, (size_t)c->aqPoolCap * (2 * sizeof(t4_overlap) + sizeof(int32_t)), hipHostMallocMapped))) return r;
  }
  const size_t rec = (size_t)c->aqPoolCap;
  if (q.wantCands && !c->candPool) {
    if (!c->candCap) c->candCap = c->aqEnv.candCap > 0 ? c->aqEnv.candCap : 1 << 18;   // (testing aid: a small pool forces the grow-and-repeat path)
    if ((r = c->candPool.alloc(c, sizeof(T4Cand) * (size_t)c->candCap, hipHostMallocMapped))) return r;
  }
  q.tf0 = std::chrono::steady_clock::now();
  auto tl_ = q.tf0;
  auto lapL = [&](int i) { const auto t = std::chrono::steady_clock::now(); c->aqSecLaunch[i] += std::chrono::duration<double>(t - tl_).count(); tl_ = t; };
  if (q.wide) {
    if ((r = ensureWide(c, q.nWideSlots, 1, 1))) return r;
    for (int half = 0; half < 2; ++half) {
      T4Wide w = wideHalf(c, half);
      w.enabled = 1; w.safetyNum = q.wideSafety; w.firstRead = w.firstPart = 0;
      // Reads of up to T4_WIDE_MIN_HITS emitted hits stay with one workgroup (LDS tier, then its slice of global scratch inside the same
      // launch, beside the other reads of the round): the wide query's kernels run behind the launch and cost a round about 0.25 ms
      // whatever the read is (profiles/r04b-h); from the LDS tier's capacity on it beats one workgroup's global scratch (C2 122 -> 93 s,
      // profiles/r04h_*). The testing aid T4_AQ_CAP_LIMIT lowers the threshold with the LDS tier's capacity.
      w.minHits = c->aqEnv.capLimit > 0 ? c->aqEnv.capLimit : c->aqEnv.wideMinHits;
      w.ctl = q.hdr.wide[half].ctl.dev(c); w.plan = q.hdr.wide[half].plan.dev(c); w.stat = q.hdr.wide[half].stat.dev(c);
      *q.in.wide[half].stage(c) = w;
    }
  }
  T4AqTail *const tail = q.hdr.tail.dev(c);
  {
    T4CandArgs cs;
    memset(&cs, 0, sizeof cs);
    cs.stats8 = q.hdr.stats8.dev(c);
    if (q.hasForce) cs.forceMin = q.in.forceMin.dev(c);
    if (q.hasArm) { cs.rorArm = q.in.arm.dev(c); cs.rorHead = q.in.head.dev(c); cs.rorInfo = q.hdr.rorInfo.dev(c); }
    if (q.keepExtAux) {   // (sized with the pool: a call repeated with a larger pool comes through here again)
      if (c->aqExtAuxCap < c->aqPoolCap) {
        c->aqExtAuxCap = 0;
        if ((r = c->aqExtAux.alloc(c, (size_t)c->aqPoolCap))) return r;
        c->aqExtAuxCap = c->aqPoolCap;
      }
      cs.extAux = c->aqExtAux;
    }
    if (q.wantCands) {
      cs.candOut = (T4Cand *)c->candPool.dev; cs.candCap = c->candCap; cs.candCursor = &tail->candCursor; cs.candOverflow = &tail->candOverflow;
      cs.candBase = q.hdr.candBase.dev(c); cs.candCnt = q.hdr.candCnt.dev(c);
    }
    *q.in.cs.stage(c) = cs;
  }
  lapL(0);
  {   // input blob into device memory, header block zeroed (counts, status, overflow lists, bases, tail): one kernel, no copy engine (t4_kernels.h: aqPrologueKernel)
    const unsigned long long inW = q.in.bytes >> 3, outW = q.hdr.bytes >> 3;
    const unsigned long long most = inW > outW ? inW : outW;
    const int grid = clampi((int)((most + 2047) / 2048), 1, c->cus * 4);
    hipLaunchKernelGGL(t4k::aqPrologueKernel, dim3(grid), dim3(256), 0, c->stream, (const unsigned long long *)c->aqInHost.dev, (unsigned long long *)c->aqIn.p, inW,
                       (unsigned long long *)c->aqOut.p, outW);
    HIPCHK(c, hipGetLastError());
  }
  lapL(1);
  T4BatchView &bv = q.bv;
  bv.pk = q.in.pk.dev(c); bv.nm = q.in.nm.dev(c); bv.len = q.in.len.dev(c);
  bv.barcode = q.in.barcode.dev(c); bv.wpk = q.wpk; bv.wnm = q.wnm; bv.n = n;
  T4QueryArgs &qa = q.qa;
  memset(&qa, 0, sizeof qa);
  qa.mode = 4; qa.skipRepeats = q.skipRepeats; qa.maxPerRead = 0;
  qa.counts = q.hdr.counts.dev(c);
  qa.out = (T4OverlapOut *)c->aqPool.dev; qa.outExt = qa.out + rec; qa.ret = (int *)(qa.outExt + rec);
  qa.outBase = q.hdr.outBase.dev(c); qa.poolCursor = &tail->poolCursor; qa.poolCap = c->aqPoolCap;
  qa.strandPerRead = q.in.strand.dev(c); qa.factorPerRead = q.in.factor.dev(c);
  qa.readTicks = q.hdr.ticks.dev(c); qa.statsStable = q.hdr.stable.dev(c); qa.aux = q.hdr.aux.dev(c); qa.n4 = q.hdr.n4.dev(c);
  if (q.hasOnly) qa.onlySeq = q.in.onlySeq.dev(c);
  qa.cs = q.in.cs.dev(c);   // statistics words always; candidate records when asked for (the struct travels in the input blob: filled before the prologue above)
  qa.leanExt = q.lean ? 1 : 0;
  if (q.views) { qa.views = q.views; qa.viewOf = q.in.viewOf.dev(c); }
  // one big set: the ExtendOverlap calls of reads with more than this many overlaps run in their own launch (0: never)
  int deferMin = c->aqEnv.extendDefer;   // testing aid
  if (q.wide && deferMin <= 0) deferMin = 16;   // the wide query leaves every ExtendOverlap to extendKernel
  const bool extendLater = deferMin > 0 && !q.views && !smallFirst && !q.onlyRestricted;
  q.extendLater = extendLater;
  if (extendLater) {
    if (c->aqRecCap < c->aqPoolCap) {
      c->aqRecCap = 0;
      if ((r = c->aqRecDev.alloc(c, (size_t)c->aqPoolCap)) || (r = c->aqRecRead.alloc(c, (size_t)c->aqPoolCap))) return r;
      c->aqRecCap = c->aqPoolCap;
    }
    qa.extendLater = deferMin; qa.outDev = c->aqRecDev; qa.recRead = c->aqRecRead;
  }
  const int threads = !smallFirst ? 512 : 256;   // workgroup of the 8192-hit tier of this path
  q.threads = threads;
  const int grid0 = smallFirst ? (n < c->cus * TIER_BLOCKS_PER_CU[0] ? n : c->cus * TIER_BLOCKS_PER_CU[0])
                               : (nFirst > 0 ? (nFirst < c->cus * 2 ? nFirst : c->cus * 2) : 1);   // persistent grid: a large batch strides (and the per-block global scratch stays bounded)
  // scratch of the fallback DPs: the blocks of the LDS launch first, those of a concurrent global-tier launch behind them
  if ((r = ensureScratch(c, (grid0 > c->cus * 2 ? grid0 : c->cus * 2) * threads + (q.wide ? (nDirect > 0 ? c->cus * 512 : 0) : nDirect * G_THREADS)))) return r;
  T4Work &wk = q.wk;
  memset(&wk, 0, sizeof wk);
  wk.list = q.in.list.dev(c); wk.nList = nFirst;
  wk.nextList = q.hdr.next.dev(c); wk.nextCount = &tail->overflow;
  wk.status = q.hdr.status.dev(c); wk.hitCounter = &tail->hits;
  wk.dpRows = c->dpRows; wk.dpDir = c->dpDir;
  wk.capLimit = c->aqEnv.capLimit;   // testing aid
  wk.wide = q.wide ? q.in.wide[0].dev(c) : nullptr;
  if (!smallFirst && (r = ensureGlobalTier(c, grid0 + (q.wide ? 0 : nDirect)))) return r;   // before anything of this call runs: growing it frees the old arrays
  lapL(0);
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  lapL(5);
  if (nDirect > 0) {   // beside the LDS tier, on the second stream (its own blocks of the DP scratch)
    if (!c->stream2) { HIPCHK(c, c->stream2.create()); HIPCHK(c, c->evIn.create()); HIPCHK(c, c->evG.create()); }
    HIPCHK(c, hipEventRecord(c->evIn, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->evIn, 0));
    T4Work wd = wk;
    wd.list = wk.list + nFirst; wd.nList = nDirect; wd.nextList = nullptr; wd.nextCount = nullptr;
    wd.dpRows = c->dpRows + (size_t)((grid0 > c->cus * 2 ? grid0 : c->cus * 2) * threads / 64) * (6 * T4_ROWW * 64);
    wd.dpDir = c->dpDir + (size_t)(grid0 > c->cus * 2 ? grid0 : c->cus * 2) * threads * T4_DIR_BYTES;
    if (q.wide) {
      // the wide query of the reads known to be heavy, beside the round's query kernel: seed stage, then the same five kernels on the
      // second half of the pools (wideHalf) and their own stretch of the DP scratch
      const T4Wide &wa = *q.in.wide[1].stage(c);
      launchWideSeed(c, c->stream2, wa, wd, wd.list, nDirect, q.skipRepeats ? 1 : 0);
      launchWide(c, c->stream2, wa, wd, wideGridParts(c, 2 * c->wideRecentParts + 4 * nDirect + 4), wideGridReads(c, nDirect));
    } else {
      wd.gKeys = c->gKeys; wd.gPairs = c->gPairs; wd.gCand = nullptr; wd.gOv = c->gOv; wd.gFin = c->gFin; wd.gOrd = c->gOrd;
      wd.gCap = G_CAP; wd.gMaxOv = G_MAXOV;
      launchTier<0, 0, G_THREADS>(nDirect, c->stream2, q.base, bv, wd, qa);
      ++c->aqGlobalLaunches; c->aqGlobalReads += nDirect;
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->evG, c->stream2));
  }
  lapL(2);
  if (nFirst > 0) {
    if (smallFirst) launchTier<1024, 128, 256>(grid0, c->stream, q.base, bv, wk, qa);
    else {   // a read that outgrows the LDS arrays goes on in global scratch inside the same launch
      T4Work wf = wk;
      const size_t skip = q.wide ? 0 : (size_t)nDirect;   // the blocks of a concurrent global-tier launch own the first slices
      wf.gKeys = c->gKeys + skip * G_CAP; wf.gPairs = c->gPairs + skip * G_CAP * 2; wf.gCand = nullptr;
      wf.gOv = c->gOv + skip * G_MAXOV * 10; wf.gFin = c->gFin + skip * G_MAXOV * 10; wf.gOrd = c->gOrd + skip * G_MAXOV;
      wf.gCap = G_CAP; wf.gMaxOv = G_MAXOV;
      launchTier<8192, 512, 512>(grid0, c->stream, q.base, bv, wf, qa);
    }
    HIPCHK(c, hipGetLastError());
  }
  lapL(3);
  if (nDirect > 0) HIPCHK(c, hipStreamWaitEvent(c->stream, c->evG, 0));   // the second stream's records are in the pool before the extensions run
  // The wide query of the reads the launch above deferred. Since round 5 a fresh heavy read is recognised on the host a round ahead and
  // starts on the second stream, so the query kernel defers a read in one whole-query round of twenty (config C2: 2 434 of 42 654): the
  // five kernels behind it were five empty grids in the others. They are launched when the header says that a read was deferred (aqEnd).
  q.lazyDone = false; q.lazyStage = false; q.sweep2Done = false;
  if (extendLater && (r = launchExtend(c, 0))) return r;   // all records of the batch
  lapL(4);
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  lapL(5);
  r = aqLaunchEpilogue(c);
  lapL(6);
  return r;
}

// The call's results are on the host once the epilogue's word holds the call's number. The caller sits on the ordered chain's critical
// path: it polls (a blocking wait wakes up tens of microseconds after the kernels are done; a round is a few hundred). Every 2^16 polls
// -- a fraction of a millisecond -- the stream itself is asked, so that a kernel that died is an error and not a wait without end.
int aqWait(t4_ctx *c) {
  const unsigned want = c->aqSeq;
  for (unsigned long long spin = 1;; ++spin) {
    if (__atomic_load_n(c->aqFlag.p, __ATOMIC_ACQUIRE) == want) return T4_OK;
    if ((spin & 0xFFFFull) == 0) {
      const hipError_t e = hipStreamQuery(c->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(c->aqFlag.p, __ATOMIC_ACQUIRE) == want) return T4_OK;
        return fail(c, T4_ERR_HIP, "the stream of an AddRead query call is idle but its epilogue never reported (word %u, expected %u)", *c->aqFlag.p, want);
      }
      if (e != hipErrorNotReady) return fail(c, T4_ERR_HIP, "AddRead query call: %s", hipGetErrorString(e));
    }
  }
}

// has the call in flight finished on the device? (1 yes or nothing in flight, 0 not yet)
int aqDone(t4_ctx *c) {
  if (!c->aq.active) return 1;
  return __atomic_load_n(c->aqFlag.p, __ATOMIC_ACQUIRE) == c->aqSeq ? 1 : 0;
}

// A launch that aqEnd adds to the call once its header is on the host: between the ctx's two events, with the extensions of the
// records it adds behind it.
template <class Launch> int aqTimedLaunch(t4_ctx *c, Launch launchIt) {
  const int recsBefore = (int)c->aq.hdr.tail.host(c)->poolCursor;
  int r;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  launchIt();
  HIPCHK(c, hipGetLastError());
  if (c->aq.extendLater && (r = launchExtend(c, recsBefore))) return r;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  return T4_OK;
}
// ... as one more stage of the call (the wide query of deferred reads, the second sweep): a new epilogue behind it, and aqEnd waits again
template <class Launch> int aqStage(t4_ctx *c, Launch launchIt) {
  c->aq.lazyStage = true;
  const int r = aqTimedLaunch(c, launchIt);
  return r ? r : aqLaunchEpilogue(c);
}
// ... as a rerun of reads on the next tier (rare paths, synchronous): the header is copied back and waited for here
template <class Launch> int aqRerun(t4_ctx *c, Launch launchIt) {
  int r;
  if ((r = aqTimedLaunch(c, launchIt))) return r;
  HIPCHK(c, hipMemcpyAsync(c->aqOutHost, c->aqOut, c->aq.hdr.bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  { float ms = 0; if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->aqKernelMs += ms; }
  return T4_OK;
}
// The whole call again, after the caller made room for what overflowed. `pool`: a pinned pool to drop (aqLaunch allocates it anew at
// the capacity the caller has set).
int aqRepeat(t4_ctx *c, PinnedBuf<unsigned char> *pool = nullptr) {
  if (pool) pool->free();
  ++c->aq.attempt;
  return aqLaunch(c);
}

// read slots of one half of the wide query that the call filled, by the header on the host
int wideSlots(const t4_ctx *c, int half) {
  const int n = c->aq.hdr.wide[half].ctl.host(c)[T4_WC_READS];
  return n < c->aq.nWideSlots ? n : c->aq.nWideSlots;
}
struct WideSlot { int half, slot; };   // (half < 0: none)
WideSlot findWideSlot(const t4_ctx *c, int read) {   // where the wide query served `read` in the last call
  for (int half = 0; half < 2; ++half) {
    const T4WidePlan *plan = c->aq.hdr.wide[half].plan.host(c);
    for (int s = 0, n = wideSlots(c, half); s < n; ++s) if (plan[s].read == read) return {half, s};
  }
  return {-1, 0};
}

// a pool of the wide query ran out (T4WideFlag bits of both halves): larger pools / finer partitions for the repeat of the call
int aqWideGrow(t4_ctx *c, int flags) {
  AqCall &q = c->aq;
  const int *ctl = q.hdr.wide[0].ctl.host(c), *ctlA = q.hdr.wide[1].ctl.host(c);
  int r;
  if (q.attempt >= 12 || (flags & (T4_WF_READS | T4_WF_INTERNAL))) return fail(c, T4_ERR_UNSUPPORTED, "wide query: flags %d after %d attempts", flags, q.attempt);
  if (flags & T4_WF_PARTS) {
    const int need = ctl[T4_WC_PARTS] > ctlA[T4_WC_PARTS] ? ctl[T4_WC_PARTS] : ctlA[T4_WC_PARTS];
    if (need <= c->wide.maxPart) return fail(c, T4_ERR_UNSUPPORTED, "a read of this batch needs more than %d partitions of %d k-mer hits", T4_WIDE_MAXP, c->wide.pcap);
    if ((r = ensureWide(c, q.nWideSlots, need, 1))) return r;
  }
  for (int b = 0; b < 6; ++b) if (flags & (1 << b)) ++c->wideFlagCounts[b];
  if (flags & (T4_WF_KEYS | T4_WF_OVERLAPS)) {
    if (q.wideSafety >= 32 * 256) return fail(c, T4_ERR_UNSUPPORTED, "wide query: a contig range of one contig overflows a partition");
    q.wideSafety *= 2;
    // keys: the partitions are quantiles of a SAMPLE of the hits' contigs; when a sample misjudged one, the next calls (the same
    // reads again, mostly) are planned less full as well. Overlaps of a partition: one read's matter (hundreds of short chains in
    // one contig range) -- finer partitions for this call only.
    if (flags & T4_WF_KEYS) { c->wideSafetyKeep = q.wideSafety < 128 ? q.wideSafety : 128; c->wideCallsSinceRepeat = 0; }
  }
  if ((flags & T4_WF_GROUPS) && (r = ensureWide(c, q.nWideSlots, 1, ctl[T4_WC_GROUPS] > ctlA[T4_WC_GROUPS] ? ctl[T4_WC_GROUPS] : ctlA[T4_WC_GROUPS]))) return r;
  ++c->wideRetries;
  return T4_OK;
}
// the wide query of a finished call: the ctx's statistics, and the reads to start on the second stream the next time
void aqWideAccount(t4_ctx *c) {
  AqCall &q = c->aq;
  const int *ctl = q.hdr.wide[0].ctl.host(c), *ctlA = q.hdr.wide[1].ctl.host(c);
  const int requeued = ctl[T4_WC_REQUEUED] + ctlA[T4_WC_REQUEUED];
  // (slots of first passes that found nothing were retired, T4WidePlan::read < 0: their partitions and dependency records are not counted)
  int retiredParts[2] = {0, 0}, retiredGroups = 0;
  for (int half = 0; half < 2 && requeued > 0; ++half) {
    const T4WidePlan *pl = q.hdr.wide[half].plan.host(c);
    const int *st = q.hdr.wide[half].stat.host(c);
    for (int s = 0, ns = wideSlots(c, half); s < ns; ++s) if (pl[s].read < 0) { retiredParts[half] += pl[s].P; retiredGroups += st[(size_t)s * T4_WIDE_STAT + WS_GROUPS]; }
  }
  c->wideReads += ctl[T4_WC_READS] + ctlA[T4_WC_READS] - requeued; c->wideParts += ctl[T4_WC_PARTS] + ctlA[T4_WC_PARTS] - retiredParts[0] - retiredParts[1];
  c->wideGroups += ctl[T4_WC_GROUPS] + ctlA[T4_WC_GROUPS] - retiredGroups;
  ++c->wideCalls; if (ctl[T4_WC_READS] > 0) ++c->wideCallsDeferred; if (ctlA[T4_WC_READS] > 0) ++c->wideCallsDirect;
  if (ctl[T4_WC_READS] + ctlA[T4_WC_READS] > 0 && ++c->wideCallsSinceRepeat >= 2048 && c->wideSafetyKeep > 32) { c->wideSafetyKeep /= 2; c->wideCallsSinceRepeat = 0; }
  { const int parts = ctl[T4_WC_PARTS] - retiredParts[0]; c->wideRecentParts = parts > c->wideRecentParts ? parts : (c->wideRecentParts * 7 + parts) / 8; }
  if (!q.tierHint) return;
  for (int half = 0; half < 2; ++half) {   // remembered by the caller: these reads start on the second stream the next time they are queried
    const T4WidePlan *pl = q.hdr.wide[half].plan.host(c);
    for (int s = 0, ns = wideSlots(c, half); s < ns; ++s) if (pl[s].read >= 0 && pl[s].read < q.n) q.tierHint[pl[s].read] = 1;
  }
}

int aqEnd(t4_ctx *c, AqResult *res) {
  AqCall &q = c->aq;
  if (!q.active) return fail(c, T4_ERR_STATE, "no AddRead query in flight on this ctx");
  q.active = false;
  (void)hipSetDevice(c->device);
  const int n = q.n;
  const bool smallFirst = q.smallFirst;
  const AqHeader &hdr = q.hdr;
  const T4AqTail *const tail = hdr.tail.host(c);   // (the header on the host: fresh after every wait below)
  const int *const ctl = hdr.wide[0].ctl.host(c), *const ctlA = hdr.wide[1].ctl.host(c);
  const T4Work &wk = q.wk;
  int r;
  for (;;) {
    // The caller sits on the ordered chain's critical path: poll for the round's last event before the blocking wait (a wait that
    // sleeps wakes up tens of microseconds after the kernels are done; a round is a few hundred)
    if ((r = aqWait(c))) return r;
    // (everything queued on the stream before the epilogue is done: what a wait for the stream said before. The runtime is told now and
    // then too, so that it retires what it keeps per command.)
    if ((c->aqSeq & 255u) == 0) HIPCHK(c, hipStreamSynchronize(c->stream));
    ++c->syncEpoch;
    {
      float ms = 0;
      hipError_t ee = hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
      if (ee == hipErrorNotReady) { (void)hipEventSynchronize(c->ev[1]); ee = hipEventElapsedTime(&ms, c->ev[0], c->ev[1]); }
      if (ee == hipSuccess) { c->aqKernelMs += ms; c->aqLastMs = q.lazyStage ? c->aqLastMs + ms : ms; }
    }
    const bool wideClean = q.wide && !ctl[T4_WC_FLAGS] && !ctlA[T4_WC_FLAGS];
    if (q.wide && !q.lazyDone) {   // did the query kernel defer a read? then its wide query runs now, and the extensions of its records behind it
      q.lazyDone = true;
      if (wideClean && ctl[T4_WC_READS] > 0) {   // (the counts of deferred reads and their partitions size the grids)
        r = aqStage(c, [&] { launchWide(c, c->stream, *q.in.wide[0].stage(c), wk, wideGridParts(c, ctl[T4_WC_PARTS] + 1), wideGridReads(c, ctl[T4_WC_READS])); });
        if (r) return r;
        continue;
      }
    }
    if (q.wide && q.skipRepeats && !q.sweep2Done) {
      // First passes of skipRepeats queries that ended without a raw overlap (wideMergeKernel queued their reads): the plain pass of
      // GetOverlapsFromRead (SeqSet.hpp:1533-1556) as a second sweep of the wide kernels -- seed stage of the queued reads of both halves
      // into fresh slots of half 0, the five kernels from those slots on, the extensions of the new records. One such sweep per attempt.
      q.sweep2Done = true;
      const int nq[2] = {ctl[T4_WC_REQUEUED], ctlA[T4_WC_REQUEUED]}, nqAll = nq[0] + nq[1];
      if (wideClean && nqAll > 0) {
        T4Wide w = *q.in.wide[0].stage(c);
        const int *const lists[2] = {w.requeue, q.in.wide[1].stage(c)->requeue};
        w.firstRead = ctl[T4_WC_READS]; w.firstPart = ctl[T4_WC_PARTS];
        r = aqStage(c, [&] {
          for (int half = 0; half < 2; ++half) if (nq[half] > 0) launchWideSeed(c, c->stream, w, wk, lists[half], nq[half], 0);
          launchWide(c, c->stream, w, wk, wideGridParts(c, 2 * c->wideRecentParts + 4 * nqAll + 4), wideGridReads(c, nqAll));
        });
        if (r) return r;
        continue;
      }
    }
    int overflow = tail->overflow;
    if (!smallFirst && tail->servedGlobal > 0) { c->aqGlobalReads += tail->servedGlobal; ++c->aqGlobalLaunches; }
    c->aqSecFirst += secondsSince(q.tf0);
    const auto tg0 = std::chrono::steady_clock::now();
    const AqField<int> *overflowList = &hdr.next;
    if (overflow > 0 && smallFirst) {   // reads beyond the 1024-hit tier: 8192-hit LDS tier
      T4Work w1 = wk;
      w1.list = hdr.next.dev(c); w1.nList = overflow;
      w1.nextList = hdr.next2.dev(c); w1.nextCount = &hdr.tail.dev(c)->overflow2;
      if ((r = ensureScratch(c, (overflow > c->cus * 2 ? overflow : c->cus * 2) * q.threads))) return r;
      w1.dpRows = c->dpRows; w1.dpDir = c->dpDir;
      if ((r = aqRerun(c, [&] { launchTier<8192, 512, 256>(overflow, c->stream, q.base, q.bv, w1, q.qa); }))) return r;
      overflow = tail->overflow2;
      overflowList = &hdr.next2;
    }
    ++c->aqCalls; c->aqReads += n;
    if (overflow > 0 && q.tierHint) {   // remembered by the caller for the next query of these reads
      const int *lst = overflowList->host(c);
      for (int t = 0; t < overflow; ++t) q.tierHint[lst[t]] = 1;
    }
    if (overflow > 0) {   // reads beyond the LDS tiers: global-scratch tier
      ++c->aqGlobalLaunches; c->aqGlobalReads += overflow;
      if ((r = ensureGlobalTier(c, overflow))) return r;
      if ((r = ensureScratch(c, (overflow > c->cus * 2 ? overflow : c->cus * 2) * G_THREADS))) return r;
      T4Work w2 = wk;
      w2.list = overflowList->dev(c); w2.nList = overflow; w2.nextList = nullptr; w2.nextCount = nullptr;
      w2.gKeys = c->gKeys; w2.gPairs = c->gPairs; w2.gCand = nullptr; w2.gOv = c->gOv; w2.gFin = c->gFin; w2.gOrd = c->gOrd;
      w2.gCap = G_CAP; w2.gMaxOv = G_MAXOV;
      w2.dpRows = c->dpRows; w2.dpDir = c->dpDir;
      if ((r = aqRerun(c, [&] { launchTier<0, 0, G_THREADS>(overflow, c->stream, q.base, q.bv, w2, q.qa); }))) return r;
    }
    c->aqSecGlobal += secondsSince(tg0);
    if (q.wide) {
      if (const int flags = ctl[T4_WC_FLAGS] | ctlA[T4_WC_FLAGS]) {   // a pool of the wide query ran out: the whole call again
        if ((r = aqWideGrow(c, flags)) || (r = aqRepeat(c))) return r;
        continue;
      }
      aqWideAccount(c);
    }
    const int *status = hdr.status.host(c);
    bool poolFull = false;
    for (int i = 0; i < n; ++i) {
      if (status[i] == 3) poolFull = true;
      else if (status[i] == 5) continue;   // a restricted re-query that one workgroup's arrays could not hold: reported to the caller (t4_add_query_last_aux)
      else if (status[i]) return fail(c, T4_ERR_UNSUPPORTED, "read %d exceeds the engine limits (status %d: %s)", i, status[i],
                                      status[i] == 2 ? "more k-mer hits or overlaps than the global tier holds" : "a posting list beyond 10000 entries, or gap DP or contig count beyond scratch");
    }
    if (tail->dirOverflow) return fail(c, T4_ERR_UNSUPPORTED, "an overhang alignment of this batch exceeds the extension kernel's direction buffer");
    if (q.wantCands && tail->candOverflow) {   // more candidate records than their pool holds: a larger pool, and the whole call again
      if (q.attempt >= 12) return fail(c, T4_ERR_UNSUPPORTED, "candidate pool of %d records overflows", c->candCap);
      while ((unsigned)c->candCap < tail->candCursor && c->candCap < (1 << 29)) c->candCap *= 2;
      c->candCap *= 2;
      ++c->candGrows;
      if ((r = aqRepeat(c, &c->candPool))) return r;
      continue;
    }
    if (poolFull) {   // more result records than the pool holds: a larger pool, and the whole call again
      if (q.attempt >= 8) return fail(c, T4_ERR_UNSUPPORTED, "result pool of %d records overflows", c->aqPoolCap);
      c->aqPoolCap *= 4; ++c->aqPoolGrows;
      if ((r = aqRepeat(c, &c->aqPool))) return r;
      continue;
    }
    const size_t rec = (size_t)c->aqPoolCap;
    c->aqRecords += tail->poolCursor;
    c->aqDeferredReads += tail->deferred;
    if (q.wantCands) c->candRecords += tail->candCursor;
    c->aqHits += (int64_t)tail->hits;
    c->aqLastTicks = hdr.ticks.host(c); c->aqLastN = n;
    c->aqLastStable = hdr.stable.host(c);
    res->counts = hdr.counts.host(c); res->base = hdr.outBase.host(c);
    res->ov = (const t4_overlap *)c->aqPool.p; res->ext = res->ov + rec; res->ret = (const int32_t *)(res->ext + rec);
    return T4_OK;
  }
}

int addQueryPool(t4_ctx *c, const T4IndexView &base, const T4IndexView *views, const int32_t *viewOf, bool smallFirst, int n, const char *bases,
                 const int64_t *offsets, const int32_t *barcodes, const int32_t *strands, int skip_repeats, const double *factors, AqResult *res,
                 unsigned char *tierHint = nullptr, bool lean = false) {
  int r = aqBegin(c, base, views, viewOf, smallFirst, n, bases, offsets, barcodes, strands, skip_repeats, factors, tierHint, lean);
  if (r) return r;
  return aqEnd(c, res);
}

// the same with the fixed-stride result layout of t4_add_query / t4_cellstore_query
int addQueryImpl(t4_ctx *c, const T4IndexView &base, const T4IndexView *views, const int32_t *viewOf, bool smallFirst, int n, const char *bases,
                 const int64_t *offsets, const int32_t *barcodes, const int32_t *strands, int skip_repeats, const double *factors,
                 int max_per_read, int32_t *counts, t4_overlap *ov, t4_overlap *ext, int32_t *ext_ret, bool lean = false) {
  AqResult res;
  int r = addQueryPool(c, base, views, viewOf, smallFirst, n, bases, offsets, barcodes, strands, skip_repeats, factors, &res, nullptr, lean);
  if (r) return r;
  for (int i = 0; i < n; ++i) {
    counts[i] = res.counts[i];
    if (res.counts[i] > max_per_read) return fail(c, T4_ERR_UNSUPPORTED, "read %d has %d overlaps, the caller made room for %d", i, res.counts[i], max_per_read);
    const int k2 = res.counts[i] > 0 ? res.counts[i] : 0;
    if (!k2) continue;
    const size_t at = (size_t)i * max_per_read;
    memcpy(ov + at, res.ov + res.base[i], sizeof(t4_overlap) * k2);
    memcpy(ext + at, res.ext + res.base[i], sizeof(t4_overlap) * k2);
    memcpy(ext_ret + at, res.ret + res.base[i], sizeof(int) * k2);
  }
  return T4_OK;
}

// Pass 2 of t4_assign_wide: the reads `todo` of the batch through the AddRead query path (GetOverlapsFromRead(read, strand, barcode,
// 0, false) and the ExtendOverlap of every overlap, factor 1.0 / 2.0 by barcode -- what AssignRead runs), which has the wide query
// behind it, and AssignRead's pick over the records of every read on the device (assignPickKernel). The batch holds the reads
// packed; the query path takes characters, so the packed words come back once.
int assignWidePass2(t4_index *ix, t4_batch *b, const std::vector<int64_t> &todo, int strand, const int32_t *strands, int32_t *ret, t4_overlap *out) {
  t4_ctx *c = ix->ctx;
  const size_t n = (size_t)b->n, wpk = (size_t)b->wpk, wnm = (size_t)b->wnm;
  std::vector<unsigned> pk(n * wpk), nm(n * wnm);
  std::vector<int> len(n), bc;
  HIPCHK(c, hipMemcpy(pk.data(), b->dPk, sizeof(unsigned) * pk.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(nm.data(), b->dNm, sizeof(unsigned) * nm.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(len.data(), b->dLen, sizeof(int) * n, hipMemcpyDeviceToHost));
  if (b->dBarcode) { bc.resize(n); HIPCHK(c, hipMemcpy(bc.data(), b->dBarcode, sizeof(int) * n, hipMemcpyDeviceToHost)); }
  DevBuf<int> dRet;
  DevBuf<T4OverlapOut> dOut;
  int r;
  if ((r = dRet.alloc(c, ASSIGN_WIDE_BATCH)) || (r = dOut.alloc(c, ASSIGN_WIDE_BATCH))) return r;
  std::string bases;
  std::vector<int64_t> off;
  std::vector<int32_t> bcs, sts, hRet(ASSIGN_WIDE_BATCH);
  std::vector<double> factors;
  std::vector<t4_overlap> hOut(ASSIGN_WIDE_BATCH);
  for (size_t at = 0; at < todo.size(); at += ASSIGN_WIDE_BATCH) {
    const int m = (int)(todo.size() - at < (size_t)ASSIGN_WIDE_BATCH ? todo.size() - at : (size_t)ASSIGN_WIDE_BATCH);
    bases.clear(); off.assign(1, 0); bcs.clear(); sts.clear(); factors.clear();
    for (int j = 0; j < m; ++j) {
      const size_t i = (size_t)todo[at + j];
      const unsigned *p = pk.data() + i * wpk, *q = nm.data() + i * wnm;
      for (int x = 0; x < len[i]; ++x) bases.push_back(((q[x >> 5] >> (x & 31)) & 1u) ? 'N' : "ACGT"[(p[x >> 4] >> ((x & 15) * 2)) & 3u]);
      off.push_back((int64_t)bases.size());
      const int barcode = bc.empty() ? -1 : bc[i];
      bcs.push_back(barcode); sts.push_back(strands ? strands[i] : strand); factors.push_back(barcode == -1 ? 1.0 : 2.0);
    }
    if ((r = aqBegin(c, ix->view, nullptr, nullptr, false, m, bases.c_str(), off.data(), bc.empty() ? nullptr : bcs.data(), sts.data(), 0, factors.data(),
                     nullptr, false, nullptr, nullptr, 2))) return r;
    AqResult res;
    if ((r = aqEnd(c, &res))) return r;
    const AqCall &q = c->aq;
    const size_t rec = (size_t)c->aqPoolCap;
    const T4OverlapOut *ov = (const T4OverlapOut *)c->aqPool.dev;
    launch(t4k::assignPickKernel, m, T4_PICK_THREADS, c->stream, m, q.hdr.counts.dev(c), q.hdr.outBase.dev(c), q.in.len.dev(c), ov,
           ov + rec, (const int *)(ov + 2 * rec), c->aqExtAux, c->aqPoolCap, dRet, dOut);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hRet.data(), dRet, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hOut.data(), dOut, sizeof(t4_overlap) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ++c->syncEpoch;
    for (int j = 0; j < m; ++j) {
      if (ret) ret[todo[at + j]] = hRet[j];
      if (out) out[todo[at + j]] = hOut[j];
    }
  }
  return T4_OK;
}
}  // namespace

extern "C" {

int t4_add_query_stats(t4_ctx *c, int64_t *out5) {   // 7 values
  if (!c || !out5) return T4_ERR_ARG;
  out5[0] = c->aqCalls; out5[1] = c->aqReads; out5[2] = c->aqGlobalLaunches; out5[3] = c->aqGlobalReads; out5[4] = c->aqRecords;
  out5[5] = (int64_t)(c->aqKernelMs * 1e3); out5[6] = c->aqHits;
  if (getenv("T4_TIMING")) fprintf(stderr, "timing: AddRead query path host seconds: pack %.3f, first launch to sync %.3f, overflow tiers %.3f; result pool grown %d times\n", c->aqSecPack, c->aqSecFirst, c->aqSecGlobal, c->aqPoolGrows);
  if (getenv("T4_TIMING")) fprintf(stderr, "timing: AddRead query path, host seconds inside the launch: preparation %.3f, prologue %.3f, second stream %.3f, query kernel %.3f, wide + extension %.3f, two event records %.3f, epilogue %.3f\n",
                                   c->aqSecLaunch[0], c->aqSecLaunch[1], c->aqSecLaunch[2], c->aqSecLaunch[3], c->aqSecLaunch[4], c->aqSecLaunch[5], c->aqSecLaunch[6]);
  if (getenv("T4_TIMING")) fprintf(stderr, "timing: wide query: %lld calls with the wide pipeline behind the query kernel, %lld of them had a read deferred to it; %lld with reads on the second stream\n", (long long)c->wideCalls, (long long)c->wideCallsDeferred, (long long)c->wideCallsDirect);
  if (getenv("T4_TIMING")) fprintf(stderr, "timing: wide query: %lld calls repeated -- partition pool %lld, keys of a partition %lld, overlaps of a partition %lld, dependency records %lld; partitions planned %d/16 full at the end\n",
                                   (long long)c->wideRetries, (long long)c->wideFlagCounts[1], (long long)c->wideFlagCounts[2], (long long)c->wideFlagCounts[3], (long long)c->wideFlagCounts[4], 16 * 16 / (c->wideSafetyKeep > 0 ? c->wideSafetyKeep : 32));
  return T4_OK;
}

// development aid (T4_ROUND_LOG): kernel milliseconds of the last AddRead query call on this ctx and, per read of that call, the
// microseconds one workgroup spent on it
int t4_add_query_last_call(t4_ctx *c, double *kernel_ms, const int32_t **ticks10ns, int *n) {
  if (!c) return T4_ERR_ARG;
  if (kernel_ms) *kernel_ms = c->aqLastMs;
  if (ticks10ns) *ticks10ns = c->aqLastTicks;
  if (n) *n = c->aqLastN;
  return T4_OK;
}

// Dependency records of read i of the last finished AddRead query call on this ctx, when the wide query served it (t4_wide.h):
// per (strand, contig) group its hits and the hull of its diagonals with three or more hits, minus-strand groups (even keys)
// first, ascending by contig within a strand. Returns 1 and the records (pinned memory, valid until the next call), 0 when the read
// was served by the LDS tier. huge: one of its lists holds more than 10000 postings; n4: groups of four or more hits.
int t4_add_query_groups(t4_ctx *c, int i, const t4_grp **groups, int *n, int *huge, int *n4) {
  if (!c || !groups || !n) return T4_ERR_ARG;
  const AqCall &q = c->aq;
  if (!q.wide || !c->aqOutHost) return 0;
  const WideSlot at = findWideSlot(c, i);
  if (at.half < 0) return 0;
  const T4WidePlan &plan = q.hdr.wide[at.half].plan.host(c)[at.slot];
  const int *st = q.hdr.wide[at.half].stat.host(c) + (size_t)at.slot * T4_WIDE_STAT;
  *groups = (const t4_grp *)c->wide.grpHost.p + (at.half ? (size_t)c->wide.grpCap : 0) + plan.grpBase;
  *n = st[WS_GROUPS];
  if (huge) *huge = plan.huge;
  if (n4) *n4 = st[WS_N4];
  return 1;
}

// The head of read i of the last finished AddRead query call on this ctx, when the wide query served it and one of its lists holds
// more than 10000 postings (`huge`): what the run test of SeqSet.hpp:931-947 reads of the read's hit array. Returns 1 with M, the
// head as a bitmap of M bits (bit k of word k / 32: entry k has a list of at most 10000 postings; pinned memory the statistics
// kernel wrote, valid until the next call) and removeOnlyRepeats of the minus strand | of the plus strand << 1; 0 for any other read
// (nothing is kept for those). M is 0 when neither flag is set: no test reads the head then.
int t4_add_query_head(t4_ctx *c, int i, int *m, const uint32_t **bits, int *ror) {
  if (!c || !m || !bits || !ror) return T4_ERR_ARG;
  const AqCall &q = c->aq;
  if (!q.wide || !c->aqOutHost || !c->wide.headHost) return 0;
  const WideSlot at = findWideSlot(c, i);
  if (at.half < 0 || !q.hdr.wide[at.half].plan.host(c)[at.slot].huge) return 0;
  const int *st = q.hdr.wide[at.half].stat.host(c) + (size_t)at.slot * T4_WIDE_STAT;
  *m = st[WS_M];
  *ror = (st[WS_ROR] ? 1 : 0) | (st[WS_ROR + 1] ? 2 : 0);
  *bits = c->wide.headHost.p + ((at.half ? (size_t)c->wide.maxReads : 0) + (size_t)at.slot) * wideHeadWords(c->wide);
  return 1;
}

// Arms the restricted re-queries of the NEXT t4_add_query_pool_begin2 call on this ctx (which must have n reads and an only_seq)
// with what the removeOnlyRepeats tests need of each read's last whole query: arm[i] = the flag of the minus strand | of the plus
// strand << 1 | 4 | M << 3 (0: read i is not armed and takes the plain restricted path), head_word[i] = first word of its head
// bitmap in `heads` (n_words words, copied). The arming is consumed by that call.
int t4_add_query_arm_long_lists(t4_ctx *c, int n, const int32_t *arm, const int32_t *head_word, const uint32_t *heads, int n_words) {
  if (!c || n < 0 || n_words < 0 || (n > 0 && (!arm || !head_word)) || (n_words > 0 && !heads)) return T4_ERR_ARG;
  c->armWords.clear(); c->armHead.clear();
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (!arm[i]) continue;
    const int m = arm[i] >> 3;
    if (!(arm[i] & 4) || m < 0 || m > 8192 || head_word[i] < 0 || (int64_t)head_word[i] + (m + 31) / 32 > n_words)
      return fail(c, T4_ERR_ARG, "t4_add_query_arm_long_lists: read %d: arm word %d, head word %d of %d", i, arm[i], head_word[i], n_words);
    any = true;
  }
  if (!any) return T4_OK;
  c->armWords.resize(2 * (size_t)n);
  for (int i = 0; i < n; ++i) { c->armWords[2 * (size_t)i] = arm[i]; c->armWords[2 * (size_t)i + 1] = arm[i] ? head_word[i] : 0; }
  c->armHead.assign(heads, heads + n_words);
  return T4_OK;
}

// per read of the last finished AddRead query call on this ctx (n entries, valid until the next call), null when the call was not
// armed: 0x100 | the group-info bits (t4_grp: bits 24-27 of cnt) of the one contig's minus group | of its plus group << 4 for an
// armed restricted re-query that was answered, 0 otherwise
int t4_add_query_last_long_lists(t4_ctx *c, const int32_t **info, int *n) {
  if (!c || !info) return T4_ERR_ARG;
  const AqCall &q = c->aq;
  *info = (q.hasArm && c->aqOutHost) ? q.hdr.rorInfo.host(c) : nullptr;
  if (n) *n = q.n;
  return T4_OK;
}

// per read of the last finished AddRead query call on this ctx (n entries, valid until the next call): aux and n4 as T4QueryArgs
// describes them, status (5: a restricted re-query that did not fit -- ask for the whole query)
int t4_add_query_last_aux(t4_ctx *c, const int32_t **aux, const int32_t **n4, const int32_t **status, int *n) {
  if (!c || !c->aqOutHost) return T4_ERR_ARG;
  const AqCall &q = c->aq;
  if (aux) *aux = q.hdr.aux.host(c);
  if (n4) *n4 = q.hdr.n4.host(c);
  if (status) *status = q.hdr.status.host(c);
  if (n) *n = q.n;
  return T4_OK;
}

// wide query of this ctx, 4 values: reads it served, partitions, calls repeated with larger pools, dependency records
int t4_add_query_wide_stats(t4_ctx *c, int64_t *out4) {
  if (!c || !out4) return T4_ERR_ARG;
  out4[0] = c->wideReads; out4[1] = c->wideParts; out4[2] = c->wideRetries; out4[3] = c->wideGroups;
  return T4_OK;
}

// reads of this ctx's AddRead query calls whose ExtendOverlap calls ran in extendKernel (more than T4_AQ_EXTEND_DEFER overlaps)
int t4_add_query_defer_stats(t4_ctx *c, int64_t *out1) {
  if (!c || !out1) return T4_ERR_ARG;
  out1[0] = c->aqDeferredReads;
  return T4_OK;
}

// per read of the last finished AddRead query call on this ctx: 1 when T4QueryArgs::statsStable says so (n entries, valid until the next call)
int t4_add_query_last_stable(t4_ctx *c, const int32_t **flags, int *n) {
  if (!c || !flags) return T4_ERR_ARG;
  *flags = c->aqLastStable;
  if (n) *n = c->aqLastN;
  return T4_OK;
}

int t4_assign_pick(t4_ctx *c, int n_reads, const int32_t *counts, const int32_t *base, const int32_t *lens, int64_t n_rec, const t4_overlap *ov,
                   const t4_overlap *ext, const int32_t *ret, const int32_t *aux, int32_t *out_ret, t4_overlap *out) {
  if (!c || n_reads < 0 || n_rec < 0 || n_rec > 0x7FFFFFFF || (n_reads > 0 && (!counts || !base || !lens || !out_ret || !out)) || (n_rec > 0 && (!ov || !ext || !ret || !aux))) return T4_ERR_ARG;
  if (n_reads == 0) return T4_OK;
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)n_reads, m = (size_t)n_rec;
  DevBuf<int> dCnt, dBase, dLen, dRet, dAux, dOutRet;
  DevBuf<T4OverlapOut> dOv, dExt, dOut;
  int r;
  if ((r = dCnt.alloc(c, n)) || (r = dBase.alloc(c, n)) || (r = dLen.alloc(c, n)) || (r = dOutRet.alloc(c, n)) || (r = dOut.alloc(c, n)) ||
      (r = dOv.alloc(c, m)) || (r = dExt.alloc(c, m)) || (r = dRet.alloc(c, m)) || (r = dAux.alloc(c, m))) return r;
  HIPCHK(c, hipMemcpy(dCnt, counts, sizeof(int) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dBase, base, sizeof(int) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dLen, lens, sizeof(int) * n, hipMemcpyHostToDevice));
  if (m) {
    HIPCHK(c, hipMemcpy(dOv, ov, sizeof(t4_overlap) * m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dExt, ext, sizeof(t4_overlap) * m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dRet, ret, sizeof(int) * m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dAux, aux, sizeof(int) * m, hipMemcpyHostToDevice));
  }
  launch(t4k::assignPickKernel, n_reads, T4_PICK_THREADS, c->stream, n_reads, dCnt, dBase, dLen, dOv, dExt, dRet, dAux, (int)n_rec, dOutRet, dOut);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out_ret, dOutRet, sizeof(int) * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(out, dOut, sizeof(t4_overlap) * n, hipMemcpyDeviceToHost));
  return T4_OK;
}

int t4_add_query_pool(t4_index *ix, int n, const char *bases, const int64_t *offsets, const int32_t *barcodes, const int32_t *strands,
                      int skip_repeats, const double *factors, const int32_t **counts, const int32_t **base, const t4_overlap **ov,
                      const t4_overlap **ext, const int32_t **ext_ret, unsigned char *tier_hint) {
  if (!ix || n <= 0 || !bases || !offsets || !strands || !factors || !counts || !base || !ov || !ext || !ext_ret) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (!ix->committed) return fail(c, T4_ERR_STATE, "index not committed");
  if (ix->view.firstIsRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_add_query needs a contig set");
  AqResult res;
  int r = addQueryPool(c, ix->view, nullptr, nullptr, false, n, bases, offsets, barcodes, strands, skip_repeats, factors, &res, tier_hint, true);
  if (r) return r;
  *counts = res.counts; *base = res.base; *ov = res.ov; *ext = res.ext; *ext_ret = res.ret;
  return T4_OK;
}

// The two halves of t4_add_query_pool: begin enqueues the call on ix's ctx and returns; the host goes on; end waits and hands the
// result out (same lifetime rules). tier_hint must stay alive until end. One call in flight per ctx.
int t4_add_query_pool_begin2(t4_index *ix, int n, const char *bases, const int64_t *offsets, const int32_t *barcodes, const int32_t *strands,
                             int skip_repeats, const double *factors, unsigned char *tier_hint, const int32_t *only_seq, const int32_t *force_min, int want_cands) {
  if (!ix || n <= 0 || !bases || !offsets || !strands || !factors) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (!ix->committed) return fail(c, T4_ERR_STATE, "index not committed");
  if (ix->view.firstIsRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_add_query needs a contig set");
  return aqBegin(c, ix->view, nullptr, nullptr, false, n, bases, offsets, barcodes, strands, skip_repeats, factors, tier_hint, true, only_seq, force_min, want_cands);   // for t4_assembler: lean records (extendOverlaps)
}
// per read of the last finished call begun with want_cands: its candidate records (cnt[i] of them from base[i] of pool, pinned
// memory valid until the next call) and its eight statistics words (T4QueryArgs::stats8)
int t4_add_query_last_cands(t4_ctx *c, const t4_cand **pool, const int32_t **base, const int32_t **cnt, const int32_t **stats8, int *n) {
  if (!c || !c->aqOutHost) return T4_ERR_ARG;
  const AqCall &q = c->aq;
  static_assert(sizeof(t4_cand) == sizeof(T4Cand) && sizeof(T4Cand) == 24 && T4_QUERY_STATS == T4_QSTATS, "candidate record layout");
  if (pool) *pool = q.wantCands ? (const t4_cand *)c->candPool.p : nullptr;
  if (base) *base = q.hdr.candBase.host(c);
  if (cnt) *cnt = q.wantCands ? q.hdr.candCnt.host(c) : nullptr;
  if (stats8) *stats8 = q.hdr.stats8.host(c);
  if (n) *n = q.n;
  return T4_OK;
}
int t4_add_query_pool_done(t4_ctx *c) { return c ? aqDone(c) : 1; }
int t4_add_query_pool_end(t4_ctx *c, const int32_t **counts, const int32_t **base, const t4_overlap **ov, const t4_overlap **ext, const int32_t **ext_ret) {
  if (!c || !counts || !base || !ov || !ext || !ext_ret) return T4_ERR_ARG;
  AqResult res;
  int r = aqEnd(c, &res);
  if (r) return r;
  *counts = res.counts; *base = res.base; *ov = res.ov; *ext = res.ext; *ext_ret = res.ret;
  return T4_OK;
}

int t4_add_query(t4_index *ix, int n, const char *bases, const int64_t *offsets, const int32_t *barcodes, const int32_t *strands,
                 int skip_repeats, const double *factors, int max_per_read, int32_t *counts, t4_overlap *ov, t4_overlap *ext, int32_t *ext_ret) {
  if (!ix || n < 0 || max_per_read <= 0 || (n > 0 && (!bases || !offsets || !strands || !factors || !counts || !ov || !ext || !ext_ret))) return T4_ERR_ARG;
  t4_ctx *c = ix->ctx;
  if (!ix->committed) return fail(c, T4_ERR_STATE, "index not committed");
  if (ix->view.firstIsRef) return fail(c, T4_ERR_UNSUPPORTED, "t4_add_query needs a contig set");
  if (n == 0) return T4_OK;
  return addQueryImpl(c, ix->view, nullptr, nullptr, false, n, bases, offsets, barcodes, strands, skip_repeats, factors, max_per_read, counts, ov, ext, ext_ret);
}

}  // extern "C"

// ---- device arena of per-barcode set images ------------------------------------------------------------------
struct t4_cellstore {
  t4_ctx *ctx = nullptr;
  int k = 9, hitLenRequired = 31, radius = 10, nomatchGapLimit = 0;
  double novelSim = 0.9;
  // The resident form's layout of a slot (t4_cellstore_stage_delta; T4DeltaRec in t4_device.h): [table: tableSlots] [postings: as
  // many as a table of tableSlots may serve] [records: seqCap] [predicate bytes | consensus | count bytes: stretchCap bytes each], contig
  // i in [off[i], off[i] + cap[i]) of each of the three blocks; stretches are handed out in the order of the contigs and never move.
  struct Resident {
    bool on = false;
    size_t tableSlots = 0, postCap = 0, oPost = 0, oSeq = 0, oPw = 0, oCons = 0, oCnt = 0, stretchCap = 0, stretchUsed = 0;
    int seqCap = 0, nseq = 0;
    std::vector<uint32_t> off, cap, len;
    std::vector<int64_t> cntSum;   // postings counted on every contig: the total of a delta is checked without the untouched contigs' bytes
  };
  struct Slot { unsigned char *base = nullptr; size_t cap = 0, imgBytes = 0; bool live = false; bool pending = false; Resident res; };
  std::vector<Slot> slots;
  std::vector<int> freeIds;
  std::vector<DevBuf<unsigned char>> chunks;   // (Slot::base and freeBySize point into these)
  size_t chunkUsed = 0;
  std::map<size_t, std::vector<unsigned char *>> freeBySize;
  DevBuf<T4IndexView> dViews;
  int viewCap = 0;
  PinnedBuf<unsigned char> stHost;   // staging of the images rebuilt since the last flush
  DevBuf<unsigned char> stDev;
  size_t stCap = 0, stUsed = 0;
  std::vector<T4CopyDesc> descs;
  DevBuf<unsigned char> dDescs;
  size_t descCap = 0;   // bytes: the descriptors of a flush and, behind them, its table builds travel in one copy
  std::vector<T4TableBuild> builds;   // tables of the compact images of this flush (t4_cellstore_stage_compact)
  std::vector<int> buildSlots;        // ... and the slot each belongs to, for the error text
  std::vector<unsigned char> ctlHost;
  std::vector<T4IndexBuild> ibuilds;   // tables and postings of the indexed images of this flush (t4_cellstore_stage_indexed)
  std::vector<int> ibuildSlots;
  // four words (device, pinned copy). [0]: 0, or 1 + the number of a table build that met a duplicate key; [2], [3]: 0, or 1 + the
  // number of an index build that gave up, and why (T4_IDXERR_*)
  DevBuf<int> dBuildErr; PinnedBuf<int> hBuildErr;
  int64_t imagesBuilt = 0, keysShipped = 0, tableBytesBuilt = 0;
  int64_t imagesIndexed = 0, countBytesShipped = 0, postingsIndexed = 0, tableBytesIndexed = 0;
  std::vector<T4DeltaApply> deltas;   // resident images of this flush, whole ones and deltas (t4_cellstore_stage_delta)
  // resident form: images staged whole, deltas, contigs shipped by deltas, deltas that did not fit their slot (the caller staged
  // the cell whole), whole images of slots that held a resident image already, postings and table bytes written on the device
  int64_t residentWhole = 0, residentDeltas = 0, deltaContigs = 0, deltaMisfits = 0, residentRestages = 0, postingsResident = 0, tableBytesResident = 0;
#ifdef T4_TEST_KNOBS
  bool dropFirstTouched = false;   // T4_TEST_DELTA_DROP: a delta loses its first touched contig on the way (the tests' negative control)
#endif
  std::vector<T4BytePatch> patches;
  DevBuf<T4BytePatch> dPatches;
  size_t patchCap = 0;
  int64_t bytesPatched = 0;
  int64_t bytesStaged = 0;
  bool bigFirst = false;   // one big set (bulk mode): reads meet hundreds of contigs, start on the 8192-hit tier
  std::mutex mu;   // t4_cellstore_stage may run on several host threads after t4_cellstore_prepare
  static constexpr size_t CHUNK = (size_t)256 << 20;
};

namespace {
int cellAlloc(t4_cellstore *cs, size_t cap, unsigned char **out) {
  auto it = cs->freeBySize.find(cap);
  if (it != cs->freeBySize.end() && !it->second.empty()) { *out = it->second.back(); it->second.pop_back(); return T4_OK; }
  if (cap > t4_cellstore::CHUNK) return fail(cs->ctx, T4_ERR_UNSUPPORTED, "a per-barcode set image of %zu bytes exceeds the arena chunk", cap);
  if (cs->chunks.empty() || cs->chunkUsed + cap > t4_cellstore::CHUNK) {
    DevBuf<unsigned char> chunk;
    if (int r = chunk.alloc(cs->ctx, t4_cellstore::CHUNK)) return r;
    cs->chunks.push_back(std::move(chunk)); cs->chunkUsed = 0;
  }
  *out = cs->chunks.back().p + cs->chunkUsed;
  cs->chunkUsed += cap;
  return T4_OK;
}
int cellStagingReserve(t4_cellstore *cs, size_t more) {
  if (cs->stUsed + more <= cs->stCap) return T4_OK;
  size_t ncap = cs->stCap ? cs->stCap : ((size_t)4 << 20);
  while (ncap < cs->stUsed + more) ncap *= 2;
  PinnedBuf<unsigned char> nh;   // (what is staged already is kept: the old pair stays until the new one stands)
  DevBuf<unsigned char> nd;
  int r;
  if ((r = nh.alloc(cs->ctx, ncap, hipHostMallocDefault)) || (r = nd.alloc(cs->ctx, ncap))) return r;
  if (cs->stUsed) memcpy(nh.p, cs->stHost.p, cs->stUsed);
  if (cs->stDev) (void)hipStreamSynchronize(cs->ctx->stream);
  cs->stHost.swap(nh); cs->stDev.swap(nd); cs->stCap = ncap;
  return T4_OK;
}
int cellFlushPatches(t4_cellstore *cs) {
  if (cs->patches.empty()) return T4_OK;
  t4_ctx *c = cs->ctx;
  if (cs->patches.size() > cs->patchCap) {
    if (cs->dPatches) (void)hipStreamSynchronize(c->stream);
    cs->patchCap = 0;
    if (int r = cs->dPatches.alloc(c, cs->patches.size() * 2)) return r;
    cs->patchCap = cs->patches.size() * 2;
  }
  HIPCHK(c, hipMemcpyAsync(cs->dPatches, cs->patches.data(), sizeof(T4BytePatch) * cs->patches.size(), hipMemcpyHostToDevice, c->stream));
  const int n = (int)cs->patches.size();
  int grid = (n + 255) / 256;
  if (grid > c->cus * 4) grid = c->cus * 4;
  hipLaunchKernelGGL(t4k::patchKernel, dim3(grid), dim3(256), 0, c->stream, (const T4BytePatch *)cs->dPatches.p, n);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host vector is reused
  cs->bytesPatched += n;
  cs->patches.clear();
  return T4_OK;
}
int cellFlush(t4_cellstore *cs) {
  if (cs->descs.empty() && cs->deltas.empty()) return cellFlushPatches(cs);
  t4_ctx *c = cs->ctx;
  // control block: [copy descriptors] [table builds] [index builds] [resident deltas], every part a multiple of 8 bytes
  const size_t descBytes = (sizeof(T4CopyDesc) * cs->descs.size() + 15) & ~(size_t)15, tblBytes = sizeof(T4TableBuild) * cs->builds.size(),
               idxBytes = sizeof(T4IndexBuild) * cs->ibuilds.size(), deltaBytes = sizeof(T4DeltaApply) * cs->deltas.size(),
               buildBytes = tblBytes + idxBytes + deltaBytes;
  if (descBytes + buildBytes > cs->descCap) {
    if (cs->dDescs) (void)hipStreamSynchronize(c->stream);
    cs->descCap = 0;
    if (int r = cs->dDescs.alloc(c, (descBytes + buildBytes) * 2)) return r;
    cs->descCap = (descBytes + buildBytes) * 2;
  }
  const unsigned char *ctl = (const unsigned char *)cs->descs.data();
  if (buildBytes) {
    cs->ctlHost.resize(descBytes + buildBytes);
    memcpy(cs->ctlHost.data(), cs->descs.data(), sizeof(T4CopyDesc) * cs->descs.size());
    if (tblBytes) memcpy(cs->ctlHost.data() + descBytes, cs->builds.data(), tblBytes);
    if (idxBytes) memcpy(cs->ctlHost.data() + descBytes + tblBytes, cs->ibuilds.data(), idxBytes);
    if (deltaBytes) memcpy(cs->ctlHost.data() + descBytes + tblBytes + idxBytes, cs->deltas.data(), deltaBytes);
    ctl = cs->ctlHost.data();
  }
  HIPCHK(c, hipMemcpyAsync(cs->stDev, cs->stHost, cs->stUsed, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(cs->dDescs, ctl, buildBytes ? descBytes + buildBytes : sizeof(T4CopyDesc) * cs->descs.size(), hipMemcpyHostToDevice, c->stream));
  if (buildBytes) {   // the tables (and the postings of the indexed images) first, then the rest of the images: they write disjoint bytes of a slot
    int r;
    if (!cs->hBuildErr && (r = cs->hBuildErr.alloc(c, 4, hipHostMallocDefault))) return r;
    if (!cs->dBuildErr) {
      if ((r = cs->dBuildErr.alloc(c, 4))) return r;
      HIPCHK(c, hipMemsetAsync(cs->dBuildErr, 0, sizeof(int) * 4, c->stream));
    }
    if (deltaBytes) {   // the touched contigs of the resident images into their stretches, ahead of the builds that read them there
      int bgrid = (int)cs->deltas.size();
      if (bgrid > c->cus * 8) bgrid = c->cus * 8;
      hipLaunchKernelGGL(t4k::cellDeltaApplyKernel, dim3(bgrid), dim3(256), 0, c->stream, (const unsigned char *)cs->stDev.p,
                         (const T4DeltaApply *)(cs->dDescs.p + descBytes + tblBytes + idxBytes), (int)cs->deltas.size());
      HIPCHK(c, hipGetLastError());
    }
    if (tblBytes) {
      int bgrid = (int)cs->builds.size();
      if (bgrid > c->cus * 8) bgrid = c->cus * 8;
      hipLaunchKernelGGL(t4k::cellTableBuildKernel, dim3(bgrid), dim3(256), 0, c->stream, (const unsigned char *)cs->stDev.p,
                         (const T4TableBuild *)(cs->dDescs.p + descBytes), (int)cs->builds.size(), cs->dBuildErr.p);
      HIPCHK(c, hipGetLastError());
    }
    if (idxBytes) {
      int bgrid = (int)cs->ibuilds.size();
      if (bgrid > c->cus * 8) bgrid = c->cus * 8;
      hipLaunchKernelGGL(t4k::cellIndexBuildKernel, dim3(bgrid), dim3(256), 0, c->stream, (const unsigned char *)cs->stDev.p,
                         (const T4IndexBuild *)(cs->dDescs.p + descBytes + tblBytes), (int)cs->ibuilds.size(), cs->dBuildErr.p + 2);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(cs->hBuildErr, cs->dBuildErr, sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (!cs->descs.empty()) {
    int grid = (int)cs->descs.size();
    if (grid > c->cus * 8) grid = c->cus * 8;
    hipLaunchKernelGGL(t4k::scatterKernel, dim3(grid), dim3(256), 0, c->stream, (const unsigned char *)cs->stDev.p, (const T4CopyDesc *)cs->dDescs.p, (int)cs->descs.size());
    HIPCHK(c, hipGetLastError());
  }
  // the pageable descriptor vector and the pinned staging are reused by the next stage() calls
  HIPCHK(c, hipStreamSynchronize(c->stream));
  cs->bytesStaged += (int64_t)cs->stUsed;
  int badSlot = -1, badIndexed = -1, why = 0;
  if (buildBytes) {
    cs->imagesBuilt += (int64_t)cs->builds.size();
    for (const T4TableBuild &tb : cs->builds) { cs->keysShipped += (int64_t)tb.nKeys; cs->tableBytesBuilt += (int64_t)(sizeof(T4HashEntC) * tb.tableSlots); }
    for (const T4IndexBuild &ib : cs->ibuilds) {
      if (ib.src) { cs->postingsResident += (int64_t)ib.npost; cs->tableBytesResident += (int64_t)(sizeof(T4HashEntC) * ib.tableSlots); continue; }
      ++cs->imagesIndexed;
      cs->countBytesShipped += (int64_t)((ib.consBytes + 15u) & ~15u); cs->postingsIndexed += (int64_t)ib.npost;
      cs->tableBytesIndexed += (int64_t)(sizeof(T4HashEntC) * ib.tableSlots);
    }
    const int e = cs->hBuildErr.p[0], ei = cs->hBuildErr.p[2];
    if (e) badSlot = (e >= 1 && e <= (int)cs->buildSlots.size()) ? cs->buildSlots[e - 1] : -2;
    if (ei) { badIndexed = (ei >= 1 && ei <= (int)cs->ibuildSlots.size()) ? cs->ibuildSlots[ei - 1] : -2; why = cs->hBuildErr.p[3]; }
    if (e || ei) {
      (void)hipMemsetAsync(cs->dBuildErr, 0, sizeof(int) * 4, c->stream);
      (void)hipStreamSynchronize(c->stream);
    }
  }
  // (a resident image whose index was refused is resident no more: its slot takes a whole image next, not a delta)
  if (badIndexed >= 0) cs->slots[badIndexed].res.on = false;
  cs->descs.clear(); cs->builds.clear(); cs->buildSlots.clear(); cs->ibuilds.clear(); cs->ibuildSlots.clear(); cs->deltas.clear(); cs->stUsed = 0;
  for (t4_cellstore::Slot &sl : cs->slots) sl.pending = false;
  if (badSlot != -1) {   // the store goes on; that slot's table is incomplete until its cell is staged again
    (void)cellFlushPatches(cs);
    return fail(c, T4_ERR_ARG, "the key records of the image of slot %d hold the same code twice", badSlot);
  }
  if (badIndexed != -1) {   // likewise: that slot's table and postings are incomplete until its cell is staged again
    (void)cellFlushPatches(cs);
    return fail(c, T4_ERR_ARG, "the index of the image of slot %d could not be built from its contigs: %s", badIndexed,
                why == T4_IDXERR_KMER ? "a counted offset has no k-mer of ACGT" : why == T4_IDXERR_FULL ? "the table of nkeys keys is too small for its distinct k-mers"
                                                                                 : "the counts do not add up to npost");
  }
  return cellFlushPatches(cs);
}
}  // namespace

extern "C" {

int t4_cellstore_create(t4_ctx *c, int k, t4_cellstore **out) {
  if (!c || !out) return T4_ERR_ARG;
  if (k < 2 || k > 31) return fail(c, T4_ERR_ARG, "kmer_length %d outside [2,31]", k);
  t4_cellstore *cs = new t4_cellstore();
  cs->ctx = c; cs->k = k;
  double kmerHitProb = pow(0.8, k);  // SeqSet::ComputeNomatchGapLimit (SeqSet.hpp:2476-2482)
  cs->nomatchGapLimit = int(k * (log(0.01) / log(1 - kmerHitProb))) + 1;
#ifdef T4_TEST_KNOBS
  cs->dropFirstTouched = getenv("T4_TEST_DELTA_DROP") != nullptr && atoi(getenv("T4_TEST_DELTA_DROP")) != 0;
#endif
  *out = cs;
  return T4_OK;
}
void t4_cellstore_destroy(t4_cellstore *cs) {
  if (!cs) return;
  (void)hipSetDevice(cs->ctx->device);
  (void)hipStreamSynchronize(cs->ctx->stream);
  delete cs;
}
int t4_cellstore_set_params(t4_cellstore *cs, int hit_len_required, int radius, double novel_sim) {
  if (!cs) return T4_ERR_ARG;
  cs->hitLenRequired = hit_len_required; cs->radius = radius; cs->novelSim = novel_sim;
  return T4_OK;
}
int t4_cellstore_open(t4_cellstore *cs, int *slot) {
  if (!cs || !slot) return T4_ERR_ARG;
  if (!cs->freeIds.empty()) { *slot = cs->freeIds.back(); cs->freeIds.pop_back(); }
  else { *slot = (int)cs->slots.size(); cs->slots.push_back(t4_cellstore::Slot()); }
  cs->slots[*slot].live = true;
  return T4_OK;
}
int t4_cellstore_close(t4_cellstore *cs, int slot) {
  if (!cs || slot < 0 || slot >= (int)cs->slots.size() || !cs->slots[slot].live) return T4_ERR_ARG;
  t4_cellstore::Slot &s = cs->slots[slot];
  if (s.base) cs->freeBySize[s.cap].push_back(s.base);
  s = t4_cellstore::Slot();
  cs->freeIds.push_back(slot);
  return T4_OK;
}

namespace {
// staged bytes of one image: its table in full (tableSlots = the table's slots) or as compact key records (tableSlots = 0)
size_t cellStagedBytes(size_t tableSlots, int nseq, int64_t nkeys, int64_t npost, int64_t cons_bytes) {
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t pwCount = (size_t)cons_bytes;   // one predicate byte per consensus byte incl. the terminators
  const size_t oPost = sizeof(T4HashEntC) * (tableSlots ? tableSlots : (size_t)nkeys), oSeq = al16(oPost + sizeof(int2) * (size_t)npost),
               oPw = al16(oSeq + sizeof(T4SeqInfo) * (size_t)nseq), oCons = al16(oPw + sizeof(T4PW) * pwCount);
  return al16(oCons + (size_t)cons_bytes + 16) + al16(sizeof(T4IndexView));
}
}  // namespace

// t4_cellstore_stage_compact: the key records of at most nkeys keys, the image from its postings on, the view
size_t t4_cellstore_image_bytes(int nseq, int64_t nkeys, int64_t npost, int64_t cons_bytes) {
  return cellStagedBytes(0, nseq, nkeys, npost, cons_bytes);
}
// t4_cellstore_stage_indexed: one count byte per consensus byte, the image from its sequence records on, the view
size_t t4_cellstore_indexed_image_bytes(int nseq, int64_t cons_bytes) {
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  return al16((size_t)cons_bytes) + cellStagedBytes(0, nseq, 0, 0, cons_bytes);
}
// t4_cellstore_stage: the whole image with its table, the view (never less than the compact form of the same cell)
size_t t4_cellstore_full_image_bytes(int nseq, int64_t nkeys, int64_t npost, int64_t cons_bytes) {
  size_t sz = 64;
  while (2 * sz < 3 * (size_t)nkeys + 2) sz <<= 1;   // load factor <= 2/3
  return cellStagedBytes(sz, nseq, nkeys, npost, cons_bytes);
}

// Serial step before a group of (possibly concurrent) t4_cellstore_stage / t4_cellstore_stage_compact calls: room for `bytes` more staged bytes and a
// view entry for every slot id up to max_slot, so that no buffer moves while images are being written.
int t4_cellstore_prepare(t4_cellstore *cs, int max_slot, size_t bytes) {
  if (!cs) return T4_ERR_ARG;
  t4_ctx *c = cs->ctx;
  (void)hipSetDevice(c->device);
  int r;
  if (max_slot >= cs->viewCap) {
    int ncap = cs->viewCap ? cs->viewCap : 1024;
    while (ncap <= max_slot) ncap *= 2;
    if ((r = cellFlush(cs))) return r;   // pending descriptors may point into the old array
    if ((r = cs->dViews.growKeep(c, cs->viewCap, ncap))) return r;
    cs->viewCap = ncap;
  }
  return cellStagingReserve(cs, bytes);
}

}  // extern "C"

namespace {
// One cell's image into staging. compact: the table travels as the (code, start, cnt) records of its keys and is built in the slot
// by cellTableBuildKernel; everything from the postings on is staged, and lands in the slot, as in the full form.
// indexed (t4_cellstore_stage_indexed): neither table nor postings travel; npostIn postings are announced, postCnt[i][o] of them at
// offset o of contig i (postCntLen[i] bytes, the rest zeros), and cellIndexBuildKernel writes both in the slot from the staged contigs.
int cellStage(t4_cellstore *cs, bool compact, int slot, int barcode, int nseq, const char *const *names, const char *const *cons,
              const int32_t *const *pw, int64_t nkeys64, const uint64_t *keyCode, const int32_t *keyBucket, const int32_t *keyCnt,
              const int32_t *postIn, int64_t *pwOffsetInImage, const int32_t *seqBarcodes, bool indexed = false, int64_t npostIn = 0,
              const uint8_t *const *postCnt = nullptr, const int32_t *postCntLen = nullptr) {
  if (!cs || slot < 0 || slot >= (int)cs->slots.size() || !cs->slots[slot].live || nseq < 0 || nkeys64 < 0) return T4_ERR_ARG;
  t4_ctx *c = cs->ctx;
  (void)hipSetDevice(c->device);
  if (nseq > T4_MAX_SEQS) return fail(c, T4_ERR_UNSUPPORTED, "more than %d sequences in one barcode", T4_MAX_SEQS);
  const size_t nkeys = (size_t)nkeys64;
  int64_t npost = 0;
  size_t nLive = 0;   // keys that own postings: the entries of the table
  if (!indexed) for (size_t i = 0; i < nkeys; ++i) { npost += keyCnt[i]; if (keyCnt[i] > 0) ++nLive; }
  else {   // refused here, before anything is queued: counts that cannot be postings of these contigs, or that are not npost of them
    if (npostIn < 0 || npostIn > 0xFFFFFFFFll || (npostIn > 0 && nkeys == 0)) return fail(c, T4_ERR_ARG, "an indexed image of %lld postings with %lld keys", (long long)npostIn, (long long)nkeys64);
    int64_t sum = 0;
    for (int i = 0; i < nseq && postCnt; ++i) {
      if (!postCnt[i]) continue;
      const int l = (int)strlen(cons[i]), n = postCntLen ? postCntLen[i] : l;
      for (int o = 0; o < n; ++o) {
        if (!postCnt[i][o]) continue;
        if (o + cs->k > l) return fail(c, T4_ERR_ARG, "postings counted at offset %d of contig %d, which has %d bases (k = %d)", o, i, l, cs->k);
        sum += postCnt[i][o];
      }
    }
    if (sum != npostIn) return fail(c, T4_ERR_ARG, "the counts of the image of slot %d add up to %lld postings, %lld were announced", slot, (long long)sum, (long long)npostIn);
    npost = npostIn;
  }
  size_t sz = 64;
  while (2 * sz < 3 * nkeys + 2) sz <<= 1;   // load factor <= 2/3
  size_t consBytes = 0, pwCount = 0;
  for (int i = 0; i < nseq; ++i) {
    size_t l = strlen(cons[i]);
    if (l > T4_MAX_SEQLEN) return fail(c, T4_ERR_UNSUPPORTED, "contig longer than %d", T4_MAX_SEQLEN);
    consBytes += l + 1; pwCount += l + 1;
  }
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t oHt = 0, oPost = al16(oHt + sizeof(T4HashEntC) * sz), oSeq = al16(oPost + sizeof(int2) * (size_t)npost),
               oPw = al16(oSeq + sizeof(T4SeqInfo) * (size_t)nseq), oCons = al16(oPw + sizeof(T4PW) * pwCount),
               blobBytes = al16(oCons + consBytes + 16);
  int r;
  const size_t viewBytes = al16(sizeof(T4IndexView));
  // staged: [key records | table] [oPost .. blobBytes of the image] [view]; indexed: [count bytes] [oSeq .. blobBytes of the image] [view]
  const size_t tailFrom = indexed ? oSeq : oPost;
  const size_t headBytes = indexed ? al16(consBytes) : compact ? sizeof(T4HashEntC) * nLive : oPost, stagedBlob = headBytes + (blobBytes - tailFrom);
  unsigned char *b = nullptr, *slotBase = nullptr;
  size_t stOff = 0;
  {
    std::lock_guard<std::mutex> lock(cs->mu);
    t4_cellstore::Slot &sl = cs->slots[slot];
    // two images of one slot in the same flush would be scattered concurrently: the caller must launch (flush) in between
    if (sl.pending) return fail(c, T4_ERR_STATE, "slot %d already has an image staged for the next launch", slot);
    sl.pending = true;
    if (blobBytes > sl.cap) {
      if (sl.base) cs->freeBySize[sl.cap].push_back(sl.base);
      size_t cap = (size_t)64 << 10;
      while (cap < blobBytes + blobBytes / 2) cap <<= 1;
      sl.base = nullptr; sl.cap = 0;
      unsigned char *p = nullptr;
      if ((r = cellAlloc(cs, cap, &p))) { sl.pending = false; return r; }   // (nothing of it is staged: the caller may stage the slot again)
      sl.base = p; sl.cap = cap;
    }
    slotBase = sl.base; sl.imgBytes = blobBytes; sl.res.on = false;   // (an image of another form: the resident layout is gone)
    if (slot >= cs->viewCap || cs->stUsed + stagedBlob + viewBytes > cs->stCap)
      return fail(c, T4_ERR_STATE, "t4_cellstore_stage without a sufficient t4_cellstore_prepare (slot %d, %zu bytes)", slot, stagedBlob + viewBytes);
    stOff = cs->stUsed;
    b = cs->stHost.p + stOff;
    T4CopyDesc d0; d0.srcOff = stOff; d0.dst = slotBase; d0.bytes = blobBytes;
    if (compact) {
      d0.srcOff = stOff + headBytes; d0.dst = slotBase + oPost; d0.bytes = blobBytes - oPost;
      T4TableBuild tb; tb.table = (T4HashEntC *)(slotBase + oHt); tb.tableSlots = sz; tb.srcOff = stOff; tb.nKeys = nLive;
      cs->builds.push_back(tb); cs->buildSlots.push_back(slot);
    }
    if (indexed) {
      d0.srcOff = stOff + headBytes; d0.dst = slotBase + oSeq; d0.bytes = blobBytes - oSeq;
      T4IndexBuild ib; ib.table = (T4HashEntC *)(slotBase + oHt); ib.post = (int2 *)(slotBase + oPost); ib.tableSlots = sz;
      ib.cntOff = stOff; ib.seqOff = stOff + headBytes; ib.consOff = stOff + headBytes + (oCons - oSeq);
      ib.consBytes = (unsigned)consBytes; ib.npost = (unsigned)npost; ib.nseq = nseq; ib.k = cs->k; ib.src = nullptr;
      cs->ibuilds.push_back(ib); cs->ibuildSlots.push_back(slot);
    }
    T4CopyDesc d1; d1.srcOff = stOff + stagedBlob; d1.dst = (unsigned char *)(cs->dViews + slot); d1.bytes = viewBytes;
    cs->descs.push_back(d0); cs->descs.push_back(d1);
    cs->stUsed += stagedBlob + viewBytes;
  }
  memset(b, 0, stagedBlob + viewBytes);
  T4HashEntC *ht = (T4HashEntC *)b;   // full: the table; compact: the key records, in the order of the keys
  if (!compact && !indexed) for (size_t t = 0; t < sz; ++t) ht[t].code = ~0ull;   // empty slots
  unsigned char *tail = b + headBytes - (tailFrom - oPost);   // where the image's byte oPost is, or would be, staged
  int2 *post = (int2 *)tail;
  const unsigned long long hashMask = sz - 1;
  size_t at = 0, kAt = 0;
  if (indexed) {   // the count bytes in the order of the consensus block: offset o of contig i at consOff(i) + o
    size_t consAt = 0;
    for (int i = 0; i < nseq; ++i) {
      const size_t l = strlen(cons[i]);
      size_t n = (postCnt && postCnt[i]) ? (postCntLen ? (size_t)(postCntLen[i] > 0 ? postCntLen[i] : 0) : l) : 0;
      if (n > l) n = l;   // (zeros beyond the contig: checked above)
      if (n) memcpy(b + consAt, postCnt[i], n);
      consAt += l + 1;
    }
  }
  for (size_t i = 0; i < (indexed ? 0 : nkeys); ++i) {
    const unsigned long long cd = keyCode[i];
    const int hb = keyBucket[i], cnt = keyCnt[i];
    for (int j = 0; j < cnt; ++j) {
      const int id = postIn[2 * (at + j)];
      if (id < 0 || id >= nseq) return fail(c, T4_ERR_ARG, "posting names sequence %d of %d", id, nseq);
      post[at + j] = make_int2(id, postIn[2 * (at + j) + 1]);
    }
    if (cnt <= 0) continue;
    if (hb != (int)((cd + (unsigned long long)(long long)(barcode + 1)) % 1000003ull)) return fail(c, T4_ERR_ARG, "key of another barcode in the image of barcode %d", barcode);
    unsigned long long s = kAt++;
    if (!compact) {
      s = t4k::mix64(cd) & hashMask;
      while (ht[s].code != ~0ull) s = (s + 1) & hashMask;
    } else if (cd == ~0ull) return fail(c, T4_ERR_ARG, "key code ~0 marks an empty table slot");
    ht[s].code = cd; ht[s].start = (unsigned)at; ht[s].cnt = (unsigned)cnt;
    at += (size_t)cnt;
  }
  T4SeqInfo *infos = (T4SeqInfo *)(tail + (oSeq - oPost));
  T4PW *pwOut = (T4PW *)(tail + (oPw - oPost));
  char *consOut = (char *)(tail + (oCons - oPost));
  size_t consAt = 0, pwAt = 0;
  for (int i = 0; i < nseq; ++i) {
    T4SeqInfo &f = infos[i];
    const int l = (int)strlen(cons[i]);
    f.consOff = (int)consAt; f.len = l; f.barcode = seqBarcodes ? seqBarcodes[i] : barcode; f.isRef = 0;
    memcpy(consOut + consAt, cons[i], (size_t)l + 1);
    consAt += (size_t)l + 1;
    char nm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    strncpy(nm, names[i], 7);
    int gt = geneType(nm);
    f.geneType = gt < 0 ? 255 : (unsigned char)gt;
    f.name0 = (unsigned char)nm[0]; f.name1 = (unsigned char)nm[1]; f.name2 = (unsigned char)nm[2]; f.name3 = (unsigned char)nm[3];
    f.pwOff = (int)pwAt;
    if (l > 0 && pw[i]) for (int t = 0; t < l; ++t) pwOut[pwAt + t] = t4PwByte(pw[i][4 * t], pw[i][4 * t + 1], pw[i][4 * t + 2], pw[i][4 * t + 3]);
    for (size_t t = (l > 0 && pw[i]) ? (size_t)l : 0; t <= (size_t)l; ++t) pwOut[pwAt + t] = t4PwByte(0, 0, 0, 0);
    pwAt += (size_t)l + 1;
  }
  if (pwOffsetInImage) *pwOffsetInImage = (int64_t)oPw;
  T4IndexView &v = *(T4IndexView *)(b + stagedBlob);
  v.k = cs->k; v.nseq = nseq; v.direct = 2; v.considerBarcode = 1;
  v.hashMask = hashMask; v.table = nullptr; v.htab = nullptr; v.ctab = (const T4HashEntC *)(slotBase + oHt); v.post = (const int2 *)(slotBase + oPost);
  v.seqs = (const T4SeqInfo *)(slotBase + oSeq); v.cons = (const char *)(slotBase + oCons); v.pw = (const T4PW *)(slotBase + oPw);
  v.radius = cs->radius; v.hitLenRequired = cs->hitLenRequired; v.nomatchGapLimit = cs->nomatchGapLimit;
  v.firstIsRef = 0; v.hasNovel = 2;
  { int maxLen = 0; for (int i = 0; i < nseq; ++i) if (infos[i].len > maxLen) maxLen = infos[i].len; v.key32 = t4Key32Bits(nseq, maxLen); }
  v.novelSim = cs->novelSim; v.refSim = 0.75; v.repeatSim = 0.95;
  return T4_OK;
}
}  // namespace

extern "C" {

int t4_cellstore_stage(t4_cellstore *cs, int slot, int barcode, int nseq, const char *const *names, const char *const *cons,
                       const int32_t *const *pw, int64_t nkeys, const uint64_t *keyCode, const int32_t *keyBucket, const int32_t *keyCnt,
                       const int32_t *postIn, int64_t *pwOffsetInImage, const int32_t *seqBarcodes) {
  return cellStage(cs, false, slot, barcode, nseq, names, cons, pw, nkeys, keyCode, keyBucket, keyCnt, postIn, pwOffsetInImage, seqBarcodes);
}
int t4_cellstore_stage_compact(t4_cellstore *cs, int slot, int barcode, int nseq, const char *const *names, const char *const *cons,
                               const int32_t *const *pw, int64_t nkeys, const uint64_t *keyCode, const int32_t *keyBucket, const int32_t *keyCnt,
                               const int32_t *postIn, int64_t *pwOffsetInImage, const int32_t *seqBarcodes) {
  return cellStage(cs, true, slot, barcode, nseq, names, cons, pw, nkeys, keyCode, keyBucket, keyCnt, postIn, pwOffsetInImage, seqBarcodes);
}
int t4_cellstore_stage_indexed(t4_cellstore *cs, int slot, int barcode, int nseq, const char *const *names, const char *const *cons,
                               const int32_t *const *pw, int64_t nkeys, int64_t npost, const uint8_t *const *postCnt, const int32_t *postCntLen,
                               int64_t *pwOffsetInImage) {
  return cellStage(cs, false, slot, barcode, nseq, names, cons, pw, nkeys, nullptr, nullptr, nullptr, nullptr, pwOffsetInImage, nullptr, true, npost, postCnt, postCntLen);
}
int t4_cellstore_indexed_stats(const t4_cellstore *cs, int64_t *out4) {
  if (!cs || !out4) return T4_ERR_ARG;
  out4[0] = cs->imagesIndexed; out4[1] = cs->countBytesShipped; out4[2] = cs->postingsIndexed; out4[3] = cs->tableBytesIndexed;
  return T4_OK;
}

}  // extern "C"

// ---- the resident form: the image stays in its slot, a change travels as the contigs it touched ---------------------------------
namespace {
inline size_t residentTableSlots(int64_t npost) {   // distinct keys <= postings: the table that serves npost keys at a load of 2/3
  size_t sz = 64;
  while (2 * sz < 3 * (size_t)npost + 2) sz <<= 1;
  return sz;
}
inline size_t residentStretch(size_t len) { return (len + 1 + 64 + 127) & ~(size_t)127; }   // room for 64 more bases, in units of 128
// 0: the delta fits the slot's resident layout; 1: it does not (a contig beyond its stretch, more contigs than records or than the
// stretches have room for, more postings than the table serves); -1: it is no delta of this image at all (reason in *why)
int residentFits(const t4_cellstore::Resident &rs, int nseq, int nTouched, const int32_t *ids, const int32_t *lens, int64_t npost, const char **why) {
  if (!rs.on) { *why = "the slot holds no resident image"; return -1; }
  if (nseq < rs.nseq) { *why = "fewer contigs than the resident image has"; return -1; }
  int fresh = 0;
  size_t used = rs.stretchUsed;
  for (int j = 0; j < nTouched; ++j) {
    const int id = ids[j];
    if (id < 0 || id >= nseq) { *why = "a touched contig id outside the cell"; return -1; }
    if (j > 0 && id <= ids[j - 1]) { *why = "touched contig ids not in ascending order"; return -1; }
    if (lens[j] < 0) { *why = "a negative contig length"; return -1; }
    if (id >= rs.nseq) { ++fresh; used += residentStretch((size_t)lens[j]); }
  }
  if (fresh != nseq - rs.nseq) { *why = "a new contig that is not among the touched ones"; return -1; }
  if (nseq > rs.seqCap || used > rs.stretchCap || npost > (int64_t)rs.postCap) return 1;
  for (int j = 0; j < nTouched; ++j) if (ids[j] < rs.nseq && (size_t)lens[j] + 1 > rs.cap[ids[j]]) return 1;
  return 0;
}
}  // namespace

extern "C" {

// staged bytes of n contigs of the resident form, whole image or delta alike, exact: their records, three blocks of len + 1 bytes
// rounded up to 16 for each, the view
size_t t4_cellstore_resident_image_bytes(int n, const int32_t *lens) {
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  size_t sz = al16(sizeof(T4DeltaRec) * (size_t)(n > 0 ? n : 0));
  for (int j = 0; j < n; ++j) sz += 3 * al16((size_t)(lens[j] > 0 ? lens[j] : 0) + 1);
  return sz + al16(sizeof(T4IndexView));
}
int t4_cellstore_delta_fits(t4_cellstore *cs, int slot, int nseq, int n_touched, const int32_t *touched_ids, const int32_t *lens, int64_t npost) {
  if (!cs || slot < 0 || slot >= (int)cs->slots.size() || n_touched < 0 || (n_touched > 0 && (!touched_ids || !lens))) return 0;
  const char *why = nullptr;
  return residentFits(cs->slots[slot].res, nseq, n_touched, touched_ids, lens, npost, &why) == 0 ? 1 : 0;
}
int t4_cellstore_stage_delta(t4_cellstore *cs, int slot, int barcode, int nseq, int n_touched, const int32_t *touched_ids, const char *const *names,
                             const char *const *cons, const int32_t *const *pw, const uint8_t *const *postCnt, const int32_t *postCntLen,
                             int64_t npost, int64_t *pwOffsets) {
  if (!cs || slot < 0 || slot >= (int)cs->slots.size() || !cs->slots[slot].live || nseq < 0 || npost < 0) return T4_ERR_ARG;
  t4_ctx *c = cs->ctx;
  (void)hipSetDevice(c->device);
  const bool whole = n_touched < 0;
  const int nT = whole ? nseq : n_touched;
  if (nT > 0 && (!names || !cons || !pw || (!whole && !touched_ids))) return T4_ERR_ARG;
  if (nseq > T4_MAX_SEQS) return fail(c, T4_ERR_UNSUPPORTED, "more than %d sequences in one barcode", T4_MAX_SEQS);
  if (npost > 0xFFFFFFFFll) return fail(c, T4_ERR_ARG, "a resident image of %lld postings", (long long)npost);
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  std::vector<int32_t> lens((size_t)nT), ids((size_t)nT);
  std::vector<int64_t> sums((size_t)nT, 0);
  for (int j = 0; j < nT; ++j) {
    const size_t l = strlen(cons[j]);
    if (l > T4_MAX_SEQLEN) return fail(c, T4_ERR_UNSUPPORTED, "contig longer than %d", T4_MAX_SEQLEN);
    lens[j] = (int32_t)l; ids[j] = whole ? j : touched_ids[j];
    if (!postCnt || !postCnt[j]) continue;
    const int n = postCntLen ? postCntLen[j] : (int)l;
    for (int o = 0; o < n; ++o) {
      if (!postCnt[j][o]) continue;
      if (o + cs->k > (int)l) return fail(c, T4_ERR_ARG, "postings counted at offset %d of contig %d, which has %d bases (k = %d)", o, ids[j], (int)l, cs->k);
      sums[j] += postCnt[j][o];
    }
  }
  const size_t viewBytes = al16(sizeof(T4IndexView)), recBytes = al16(sizeof(T4DeltaRec) * (size_t)nT);
  size_t staged = recBytes;
  for (int j = 0; j < nT; ++j) staged += 3 * al16((size_t)lens[j] + 1);
  unsigned char *b = nullptr, *slotBase = nullptr;
  size_t stOff = 0;
  int r, dropped = 0;   // (records the test knob keeps back: the kernel's offsets count from the first record it is given)
  {
    std::lock_guard<std::mutex> lock(cs->mu);
    t4_cellstore::Slot &sl = cs->slots[slot];
    t4_cellstore::Resident &rs = sl.res;
    const bool wasResident = rs.on;
    if (sl.pending) return fail(c, T4_ERR_STATE, "slot %d already has an image staged for the next launch", slot);
    int64_t total = 0;
    for (int j = 0; j < nT; ++j) total += sums[j];
    // (asked before the layout or a counter moves: a refusal leaves the slot as it was)
    const bool room = slot < cs->viewCap && cs->stUsed + staged + viewBytes <= cs->stCap;
    if (!whole) {   // refused before anything is queued or the layout is touched
      const char *why = nullptr;
      const int fit = residentFits(rs, nseq, nT, ids.data(), lens.data(), npost, &why);
      if (fit < 0) return fail(c, T4_ERR_ARG, "the delta of slot %d: %s", slot, why);
      for (int i = 0; i < rs.nseq; ++i) total += rs.cntSum[(size_t)i];
      for (int j = 0; j < nT; ++j) if (ids[j] < rs.nseq) total -= rs.cntSum[(size_t)ids[j]];
      if (total != npost) return fail(c, T4_ERR_ARG, "the counts of the image of slot %d add up to %lld postings, %lld were announced", slot, (long long)total, (long long)npost);
      if (fit > 0) { ++cs->deltaMisfits; return T4_CELL_DELTA_WHOLE; }
      if (!room) return fail(c, T4_ERR_STATE, "t4_cellstore_stage_delta without a sufficient t4_cellstore_prepare (slot %d, %zu bytes)", slot, staged + viewBytes);
    } else {
      if (total != npost) return fail(c, T4_ERR_ARG, "the counts of the image of slot %d add up to %lld postings, %lld were announced", slot, (long long)total, (long long)npost);
      // a fresh layout: spare records and spare stretch room for contigs to come
      t4_cellstore::Resident nr;
      nr.tableSlots = residentTableSlots(npost); nr.postCap = (2 * nr.tableSlots - 2) / 3;
      nr.seqCap = (nseq + 8 + 7) & ~7; nr.nseq = 0;
      size_t used = 0;
      for (int j = 0; j < nseq; ++j) used += residentStretch((size_t)lens[j]);
      nr.stretchCap = used + (size_t)(nr.seqCap - nseq) * 256;
      if (nr.stretchCap > 0x7FFFFFFFull) return fail(c, T4_ERR_UNSUPPORTED, "the contigs of one barcode exceed 2 GB");
      if (!room) return fail(c, T4_ERR_STATE, "t4_cellstore_stage_delta without a sufficient t4_cellstore_prepare (slot %d, %zu bytes)", slot, staged + viewBytes);
      nr.oPost = sizeof(T4HashEntC) * nr.tableSlots; nr.oSeq = al16(nr.oPost + sizeof(int2) * nr.postCap);
      nr.oPw = (nr.oSeq + sizeof(T4SeqInfo) * (size_t)nr.seqCap + 127) & ~(size_t)127; nr.oCons = nr.oPw + nr.stretchCap; nr.oCnt = nr.oCons + nr.stretchCap;
      const size_t blobBytes = nr.oCnt + nr.stretchCap + 16;
      if (blobBytes > sl.cap) {
        if (sl.base) cs->freeBySize[sl.cap].push_back(sl.base);
        size_t cap = (size_t)64 << 10;
        while (cap < blobBytes + blobBytes / 2) cap <<= 1;
        sl.base = nullptr; sl.cap = 0; sl.imgBytes = 0; rs.on = false;
        unsigned char *p = nullptr;
        if ((r = cellAlloc(cs, cap, &p))) return r;
        sl.base = p; sl.cap = cap;
      }
      if (wasResident) ++cs->residentRestages;
      sl.imgBytes = blobBytes;
      rs = std::move(nr); rs.on = true;
    }
    sl.pending = true;
    slotBase = sl.base;
    stOff = cs->stUsed;
    b = cs->stHost.p + stOff;
    cs->stUsed += staged + viewBytes;
    // the layout takes the touched contigs: new ones get the next stretches, in the order of their ids
    rs.off.resize((size_t)nseq); rs.cap.resize((size_t)nseq); rs.len.resize((size_t)nseq); rs.cntSum.resize((size_t)nseq, 0);
    for (int j = 0; j < nT; ++j) {
      const size_t id = (size_t)ids[j];
      if ((int)id >= rs.nseq) { rs.off[id] = (uint32_t)rs.stretchUsed; rs.cap[id] = (uint32_t)residentStretch((size_t)lens[j]); rs.stretchUsed += rs.cap[id]; }
      rs.len[id] = (uint32_t)lens[j]; rs.cntSum[id] = sums[j];
    }
    rs.nseq = nseq;
#ifdef T4_TEST_KNOBS
    if (!whole && cs->dropFirstTouched && nT > 0) dropped = 1;   // (the record and payload of the first touched contig stay behind)
#endif
    const int nShip = nT - dropped;
    T4DeltaApply da;
    da.seqs = (T4SeqInfo *)(slotBase + rs.oSeq); da.pw = slotBase + rs.oPw; da.cons = slotBase + rs.oCons; da.cnt = slotBase + rs.oCnt;
    da.view = cs->dViews + slot; da.recOff = stOff + (size_t)dropped * sizeof(T4DeltaRec); da.viewOff = stOff + staged; da.nTouched = nShip; da.pad = 0;
    cs->deltas.push_back(da);
    T4IndexBuild ib; ib.table = (T4HashEntC *)slotBase; ib.post = (int2 *)(slotBase + rs.oPost); ib.tableSlots = rs.tableSlots;
    ib.cntOff = rs.oCnt; ib.seqOff = rs.oSeq; ib.consOff = rs.oCons; ib.consBytes = (unsigned)rs.stretchUsed; ib.npost = (unsigned)npost;
    ib.nseq = nseq; ib.k = cs->k; ib.src = slotBase;
    cs->ibuilds.push_back(ib); cs->ibuildSlots.push_back(slot);
    if (whole) ++cs->residentWhole; else { ++cs->residentDeltas; cs->deltaContigs += nT; }
  }
  // (from here on the slot's layout record is read only: stage calls of other slots may run beside this one)
  const t4_cellstore::Resident &rs = cs->slots[slot].res;
  memset(b, 0, staged + viewBytes);
  T4DeltaRec *recs = (T4DeltaRec *)b;
  size_t at = recBytes;
  int maxLen = 0;
  for (int j = 0; j < nT; ++j) {
    const size_t id = (size_t)ids[j], l = (size_t)lens[j], bytes = al16(l + 1);
    T4DeltaRec &rc = recs[j];
    T4SeqInfo &f = rc.info;
    f.consOff = (int)rs.off[id]; f.len = (int)l; f.pwOff = (int)rs.off[id]; f.barcode = barcode; f.isRef = 0; f.pad1 = 0;
    char nm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    strncpy(nm, names[j], 7);
    const int gt = geneType(nm);
    f.geneType = gt < 0 ? 255 : (unsigned char)gt;
    f.name0 = (unsigned char)nm[0]; f.name1 = (unsigned char)nm[1]; f.name2 = (unsigned char)nm[2]; f.name3 = (unsigned char)nm[3];
    rc.seq = (int)id; rc.srcOff = (unsigned)(at - (size_t)dropped * sizeof(T4DeltaRec)); rc.bytes = (unsigned)bytes; rc.cap = rs.cap[id];
    T4PW *pwOut = (T4PW *)(b + at);
    if (l > 0 && pw[j]) for (size_t t = 0; t < l; ++t) pwOut[t] = t4PwByte(pw[j][4 * t], pw[j][4 * t + 1], pw[j][4 * t + 2], pw[j][4 * t + 3]);
    for (size_t t = (l > 0 && pw[j]) ? l : 0; t < bytes; ++t) pwOut[t] = t4PwByte(0, 0, 0, 0);
    memcpy(b + at + bytes, cons[j], l);
    size_t n = (postCnt && postCnt[j]) ? (postCntLen ? (size_t)(postCntLen[j] > 0 ? postCntLen[j] : 0) : l) : 0;
    if (n > l) n = l;
    if (n) memcpy(b + at + 2 * bytes, postCnt[j], n);
    at += 3 * bytes;
  }
  for (int i = 0; i < nseq; ++i) if ((int)rs.len[(size_t)i] > maxLen) maxLen = (int)rs.len[(size_t)i];
  if (pwOffsets) for (int i = 0; i < nseq; ++i) pwOffsets[i] = (int64_t)(rs.oPw + rs.off[(size_t)i]);
  T4IndexView &v = *(T4IndexView *)(b + staged);
  v.k = cs->k; v.nseq = nseq; v.direct = 2; v.considerBarcode = 1;
  v.hashMask = rs.tableSlots - 1; v.table = nullptr; v.htab = nullptr; v.ctab = (const T4HashEntC *)slotBase; v.post = (const int2 *)(slotBase + rs.oPost);
  v.seqs = (const T4SeqInfo *)(slotBase + rs.oSeq); v.cons = (const char *)(slotBase + rs.oCons); v.pw = (const T4PW *)(slotBase + rs.oPw);
  v.radius = cs->radius; v.hitLenRequired = cs->hitLenRequired; v.nomatchGapLimit = cs->nomatchGapLimit;
  v.firstIsRef = 0; v.hasNovel = 2;
  v.key32 = t4Key32Bits(nseq, maxLen);
  v.novelSim = cs->novelSim; v.refSim = 0.75; v.repeatSim = 0.95;
  return T4_OK;
}
int t4_cellstore_resident_stats(const t4_cellstore *cs, int64_t *out7) {
  if (!cs || !out7) return T4_ERR_ARG;
  out7[0] = cs->residentWhole; out7[1] = cs->residentDeltas; out7[2] = cs->deltaContigs; out7[3] = cs->deltaMisfits;
  out7[4] = cs->residentRestages; out7[5] = cs->postingsResident; out7[6] = cs->tableBytesResident;
  return T4_OK;
}

// Test and diagnostic aid: flush, then the image of the slot as it lies in the arena (its table, postings, sequence records,
// predicate bytes, consensus) and its view. *bytes is the image's size also when buf is null or cap too small (T4_ERR_ARG then).
int t4_cellstore_read_image(t4_cellstore *cs, int slot, void *buf, size_t cap, size_t *bytes, void *view) {
  if (!cs || slot < 0 || slot >= (int)cs->slots.size() || !bytes) return T4_ERR_ARG;
  t4_ctx *c = cs->ctx;
  (void)hipSetDevice(c->device);
  int r;
  if ((r = cellFlush(cs))) return r;
  const t4_cellstore::Slot &sl = cs->slots[slot];
  if (!sl.base || !sl.imgBytes || slot >= cs->viewCap) return fail(c, T4_ERR_STATE, "cell slot %d has no image", slot);
  *bytes = sl.imgBytes;
  if (buf && cap < sl.imgBytes) return fail(c, T4_ERR_ARG, "the image of slot %d has %zu bytes", slot, sl.imgBytes);
  if (buf) HIPCHK(c, hipMemcpyAsync(buf, sl.base, sl.imgBytes, hipMemcpyDeviceToHost, c->stream));
  if (view) HIPCHK(c, hipMemcpyAsync(view, cs->dViews + slot, sizeof(T4IndexView), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return T4_OK;
}
int t4_cellstore_image_stats(const t4_cellstore *cs, int64_t *out4) {
  if (!cs || !out4) return T4_ERR_ARG;
  out4[0] = cs->imagesBuilt; out4[1] = cs->keysShipped; out4[2] = cs->tableBytesBuilt; out4[3] = cs->bytesStaged + cs->bytesPatched;
  return T4_OK;
}

int t4_cellstore_patch(t4_cellstore *cs, int slot, int n, const int64_t *byteOffsets, const unsigned char *values) {
  if (!cs || slot < 0 || slot >= (int)cs->slots.size() || !cs->slots[slot].base || n < 0 || (n > 0 && (!byteOffsets || !values))) return T4_ERR_ARG;
  const t4_cellstore::Slot &sl = cs->slots[slot];
  for (int i = 0; i < n; ++i) {
    if (byteOffsets[i] < 0 || (size_t)byteOffsets[i] >= sl.cap) return fail(cs->ctx, T4_ERR_ARG, "patch outside the image of slot %d", slot);
    T4BytePatch p; p.dst = sl.base + byteOffsets[i]; p.val = values[i];
    cs->patches.push_back(p);
  }
  return T4_OK;
}

int t4_cellstore_query(t4_cellstore *cs, int n, const int32_t *slots, const char *bases, const int64_t *offsets, const int32_t *barcodes,
                       const int32_t *strands, int skip_repeats, const double *factors, int max_per_read, int32_t *counts,
                       t4_overlap *ov, t4_overlap *ext, int32_t *ext_ret) {
  if (!cs || n < 0 || max_per_read <= 0 || (n > 0 && (!slots || !bases || !offsets || !strands || !factors || !counts || !ov || !ext || !ext_ret))) return T4_ERR_ARG;
  t4_ctx *c = cs->ctx;
  (void)hipSetDevice(c->device);
  int r;
  if ((r = cellFlush(cs))) return r;
  if (n == 0) return T4_OK;
  for (int i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= (int)cs->slots.size() || !cs->slots[slots[i]].base) return fail(c, T4_ERR_STATE, "read %d names cell slot %d which has no image", i, slots[i]);
  T4IndexView base;
  memset(&base, 0, sizeof base);
  base.k = cs->k;
  return addQueryImpl(c, base, cs->dViews, slots, !cs->bigFirst, n, bases, offsets, barcodes, strands, skip_repeats, factors, max_per_read, counts, ov, ext, ext_ret, true);   // consumed by t4_assembler::addRead only: lean records
}
int t4_cellstore_set_big_first(t4_cellstore *cs, int on) { if (!cs) return T4_ERR_ARG; cs->bigFirst = on != 0; return T4_OK; }
int64_t t4_cellstore_bytes_staged(const t4_cellstore *cs) { return cs ? cs->bytesStaged + cs->bytesPatched : 0; }

}  // extern "C"

// ---- t4_comm: RCCL all-gather of byte strings between the ranks of one node (one process per GPU) -------------------------------
#ifdef __HIPCC__
// RCCL is bound when the first communicator is asked for (dlopen), not when libt4hip.so is loaded: a single-GPU host without
// librccl still loads the library and runs everything but t4_comm. <rccl/rccl.h> gives the types only.
struct RcclApi {
  void *lib = nullptr;
  decltype(&ncclGetUniqueId) getUniqueId = nullptr;
  decltype(&ncclCommInitRank) commInitRank = nullptr;
  decltype(&ncclCommDestroy) commDestroy = nullptr;
  decltype(&ncclCommAbort) commAbort = nullptr;
  decltype(&ncclCommGetAsyncError) commGetAsyncError = nullptr;
  decltype(&ncclAllGather) allGather = nullptr;
  decltype(&ncclSend) send = nullptr;
  decltype(&ncclRecv) recv = nullptr;
  decltype(&ncclGroupStart) groupStart = nullptr;
  decltype(&ncclGroupEnd) groupEnd = nullptr;
  std::string error;
};
static RcclApi *rcclApi() {
  static std::mutex mu;
  static RcclApi api;
  std::lock_guard<std::mutex> lk(mu);
  if (api.lib || !api.error.empty()) return &api;
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  void *h = nullptr;
  for (const char *nm : names) if ((h = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
  if (!h) { const char *e = dlerror(); api.error = std::string("librccl.so not found (") + (e ? e : "dlopen failed") + ")"; return &api; }
  bool ok = true;
  auto bind = [&](auto &fp, const char *sym) { fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, sym)); if (!fp) { ok = false; api.error = std::string("librccl.so lacks ") + sym; } };
  bind(api.getUniqueId, "ncclGetUniqueId"); bind(api.commInitRank, "ncclCommInitRank"); bind(api.commDestroy, "ncclCommDestroy"); bind(api.commAbort, "ncclCommAbort"); bind(api.commGetAsyncError, "ncclCommGetAsyncError");
  bind(api.allGather, "ncclAllGather"); bind(api.send, "ncclSend"); bind(api.recv, "ncclRecv");
  bind(api.groupStart, "ncclGroupStart"); bind(api.groupEnd, "ncclGroupEnd");
  if (!ok) { dlclose(h); return &api; }
  api.lib = h;
  return &api;
}
#endif

struct t4_comm {
  t4_ctx *ctx = nullptr;
  int rank = 0, nranks = 1;
#ifdef __HIPCC__
  ncclComm_t comm = nullptr;
  RcclApi *rccl = nullptr;
#endif
};

#ifdef __HIPCC__
// The wait of a collective, bounded: a rank that died before it leaves the others in the kernel RCCL enqueued for ever.
// Polls the stream; an asynchronous RCCL error or T4_COMM_TIMEOUT_S seconds (default 3600: ranks of a sharded sample may finish far
// apart) abort the communicator and come back as an error instead of a hang.
static int commWait(t4_comm *cm, const char *what, double limitS = 0) {
  t4_ctx *c = cm->ctx;
  const char *ev = getenv("T4_COMM_TIMEOUT_S");
  const double limit = limitS > 0 ? limitS : (ev && atof(ev) > 0 ? atof(ev) : 3600.0);
  const auto t0 = std::chrono::steady_clock::now();
  for (long long spin = 0;; ++spin) {
    const hipError_t q = hipStreamQuery(c->stream);
    if (q == hipSuccess) return T4_OK;
    if (q != hipErrorNotReady) return fail(c, T4_ERR_HIP, "t4_comm (%s): %s", what, hipGetErrorString(q));
    ncclResult_t ar = ncclSuccess;
    const bool asyncBad = cm->comm && (spin & 1023) == 1023 && cm->rccl->commGetAsyncError(cm->comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress;
    const bool late = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit;
    if (asyncBad || late) {
      if (cm->comm) { (void)cm->rccl->commAbort(cm->comm); cm->comm = nullptr; }
      return fail(c, T4_ERR_HIP, late ? "t4_comm (%s): rank %d of %d waited %.0f s for the other ranks (T4_COMM_TIMEOUT_S); communicator aborted" : "t4_comm (%s): RCCL reported an asynchronous error on rank %d of %d (%.0f s); communicator aborted",
                  what, cm->rank, cm->nranks, limit);
    }
    if (spin < 2000) std::this_thread::yield(); else usleep(200);
  }
}
#endif

#ifdef __HIPCC__
namespace {
// device / host buffers of one collective: released on every path out of it (the error returns leaked them)
struct CommBufs {
  std::vector<void *> dev; void *host = nullptr;
  ~CommBufs() { for (void *p : dev) if (p) (void)hipFree(p); if (host) free(host); }
  template <class T> hipError_t devAlloc(T **p, size_t bytes) { *p = nullptr; const hipError_t e = hipMalloc((void **)p, bytes ? bytes : 8); if (e == hipSuccess) dev.push_back(*p); return e; }
  void *releaseHost() { void *h = host; host = nullptr; return h; }
};
// lengths of every rank's contribution: one 8-byte ncclAllGather. The bounded wait comes BEFORE any device-to-host copy is queued: a
// copy into pageable memory runs synchronously behind the RCCL kernel, and with a dead peer the host would hang inside hipMemcpyAsync
// and never reach commWait.
int commLengths(t4_comm *cm, int64_t n, std::vector<unsigned long long> &lens) {
  t4_ctx *c = cm->ctx;
  const int R = cm->nranks;
  CommBufs bufs;
  unsigned long long *dLen = nullptr;
  HIPCHK(c, bufs.devAlloc(&dLen, sizeof(unsigned long long) * (size_t)(R + 1)));
  const unsigned long long myLen = (unsigned long long)n;
  HIPCHK(c, hipMemcpy(dLen + R, &myLen, sizeof myLen, hipMemcpyHostToDevice));
  if (cm->rccl->allGather(dLen + R, dLen, 1, ncclUint64, cm->comm, c->stream) != ncclSuccess) return fail(c, T4_ERR_HIP, "ncclAllGather (lengths) failed");
  if (int wr = commWait(cm, "the lengths")) return wr;
  lens.resize((size_t)R);
  HIPCHK(c, hipMemcpy(lens.data(), dLen, sizeof(unsigned long long) * (size_t)R, hipMemcpyDeviceToHost));
  return T4_OK;
}
}  // namespace
#endif

extern "C" {

int t4_comm_init(t4_ctx *c, int rank, int nranks, const char *id_path, t4_comm **out) {
  if (!c || !out || nranks < 1 || rank < 0 || rank >= nranks || !id_path) return T4_ERR_ARG;
#ifdef __HIPCC__
  (void)hipSetDevice(c->device);
  RcclApi *rccl = rcclApi();
  if (!rccl->lib) return fail(c, T4_ERR_UNSUPPORTED, "t4_comm: %s", rccl->error.c_str());
  ncclUniqueId id;
  if (rank == 0) {
    (void)unlink(id_path);   // (an id left by an earlier run must not be taken for this one's)
    if (rccl->getUniqueId(&id) != ncclSuccess) return fail(c, T4_ERR_HIP, "ncclGetUniqueId failed");
    const std::string tmp = std::string(id_path) + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "wb");
    if (!fp || fwrite(&id, sizeof id, 1, fp) != 1) { if (fp) fclose(fp); return fail(c, T4_ERR_IO, "cannot write %s", tmp.c_str()); }
    fclose(fp);
    if (rename(tmp.c_str(), id_path)) return fail(c, T4_ERR_IO, "cannot create %s", id_path);
  } else {
    bool got = false;
    for (int tries = 0; tries < 6000 && !got; ++tries) {   // up to ten minutes: rank 0 may still be parsing its input
      FILE *fp = fopen(id_path, "rb");
      if (fp) { got = fread(&id, sizeof id, 1, fp) == 1; fclose(fp); }
      if (!got) usleep(100000);
    }
    if (!got) return fail(c, T4_ERR_IO, "no communicator id appeared at %s", id_path);
  }
  t4_comm *cm = new t4_comm();
  cm->ctx = c; cm->rank = rank; cm->nranks = nranks; cm->rccl = rccl;
  if (rccl->commInitRank(&cm->comm, nranks, id, rank) != ncclSuccess) { delete cm; return fail(c, T4_ERR_HIP, "ncclCommInitRank(%d of %d) failed", rank, nranks); }
  // Self-check before anything depends on the communicator (RCCL had only ever run with one rank): every rank
  // contributes its number, everybody must receive 0..N-1 in order, within T4_COMM_INIT_TIMEOUT_S (default 120 s).
  {
    CommBufs bufs;
    int *d = nullptr;
    bool ok = bufs.devAlloc(&d, sizeof(int) * (size_t)(nranks + 1)) == hipSuccess && hipMemcpy(d + nranks, &rank, sizeof rank, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && rccl->allGather(d + nranks, d, 1, ncclInt32, cm->comm, c->stream) == ncclSuccess;
    const char *lim = getenv("T4_COMM_INIT_TIMEOUT_S");
    ok = ok && commWait(cm, "the self-check", lim && atof(lim) > 0 ? atof(lim) : 120.0) == T4_OK;
    std::vector<int> got((size_t)nranks, -1);
    ok = ok && hipMemcpy(got.data(), d, sizeof(int) * (size_t)nranks, hipMemcpyDeviceToHost) == hipSuccess;
    for (int r = 0; ok && r < nranks; ++r) ok = got[(size_t)r] == r;
    if (!ok) {
      if (cm->comm) (void)rccl->commAbort(cm->comm);
      delete cm;
      return fail(c, T4_ERR_HIP, "t4_comm: the self-check of the new communicator failed on rank %d of %d (a 1-int all-gather did not return the rank numbers)", rank, nranks);
    }
  }
  *out = cm;
  return T4_OK;
#else
  (void)out;
  return fail(c, T4_ERR_UNSUPPORTED, "t4_comm needs the hipcc build (RCCL)");
#endif
}


int t4_comm_allgather_bytes(t4_comm *cm, const void *mine, int64_t n, void **all, int64_t *sizes) {
  if (!cm || n < 0 || (n > 0 && !mine) || !all || !sizes) return T4_ERR_ARG;
#ifdef __HIPCC__
  t4_ctx *c = cm->ctx;
  if (!cm->comm) return fail(c, T4_ERR_ARG, "t4_comm: the communicator was aborted");
  (void)hipSetDevice(c->device);
  const int R = cm->nranks;
  // lengths first (8 bytes per rank), then the payloads padded to the longest: two ncclAllGather calls on the ctx's stream
  std::vector<unsigned long long> lens;
  if (int r = commLengths(cm, n, lens)) return r;
  size_t cap = 8, total = 0;
  for (int r = 0; r < R; ++r) { sizes[r] = (int64_t)lens[(size_t)r]; total += (size_t)lens[(size_t)r]; if ((size_t)lens[(size_t)r] > cap) cap = (size_t)lens[(size_t)r]; }
  cap = (cap + 7) & ~(size_t)7;
  CommBufs bufs;
  unsigned char *dSend = nullptr, *dRecv = nullptr;
  HIPCHK(c, bufs.devAlloc(&dSend, cap));
  if (bufs.devAlloc(&dRecv, cap * (size_t)R) != hipSuccess) return fail(c, T4_ERR_HIP, "out of device memory for the gather");
  if (n > 0) HIPCHK(c, hipMemcpy(dSend, mine, (size_t)n, hipMemcpyHostToDevice));
  if (cm->rccl->allGather(dSend, dRecv, cap, ncclUint8, cm->comm, c->stream) != ncclSuccess) return fail(c, T4_ERR_HIP, "ncclAllGather (payload) failed");
  if (int wr = commWait(cm, "the all-gather")) return wr;   // (before the copies below: see commLengths)
  bufs.host = malloc(total ? total : 1);
  if (!bufs.host) return fail(c, T4_ERR_HIP, "out of host memory for the gather");
  size_t at = 0;
  for (int r = 0; r < R; ++r) {
    if (lens[(size_t)r]) HIPCHK(c, hipMemcpy((unsigned char *)bufs.host + at, dRecv + cap * (size_t)r, (size_t)lens[(size_t)r], hipMemcpyDeviceToHost));
    at += (size_t)lens[(size_t)r];
  }
  *all = bufs.releaseHost();
  return T4_OK;
#else
  return T4_ERR_UNSUPPORTED;
#endif
}

// The same contributions, received by `root` only (the others get *all = NULL): lengths by one small ncclAllGather, payloads by one
// group of ncclSend / ncclRecv -- nothing is padded and nothing lands on ranks that do not write the files.
int t4_comm_gather_bytes(t4_comm *cm, const void *mine, int64_t n, int root, void **all, int64_t *sizes) {
  if (!cm || n < 0 || (n > 0 && !mine) || !all || !sizes || root < 0 || root >= cm->nranks) return T4_ERR_ARG;
  *all = nullptr;
#ifdef __HIPCC__
  t4_ctx *c = cm->ctx;
  if (!cm->comm) return fail(c, T4_ERR_ARG, "t4_comm: the communicator was aborted");
  (void)hipSetDevice(c->device);
  const int R = cm->nranks;
  std::vector<unsigned long long> lens;
  if (int r = commLengths(cm, n, lens)) return r;
  size_t total = 0;
  for (int r = 0; r < R; ++r) { sizes[r] = (int64_t)lens[(size_t)r]; total += (size_t)lens[(size_t)r]; }
  CommBufs bufs;
  unsigned char *dSend = nullptr, *dRecv = nullptr;
  HIPCHK(c, bufs.devAlloc(&dSend, (size_t)n));
  if (n > 0) HIPCHK(c, hipMemcpy(dSend, mine, (size_t)n, hipMemcpyHostToDevice));
  if (cm->rank == root && bufs.devAlloc(&dRecv, total) != hipSuccess) return fail(c, T4_ERR_HIP, "out of device memory for the gather");
  bool ok = cm->rccl->groupStart() == ncclSuccess;
  if (ok && n > 0) ok = cm->rccl->send(dSend, (size_t)n, ncclUint8, root, cm->comm, c->stream) == ncclSuccess;
  if (ok && cm->rank == root) {
    size_t at = 0;
    for (int r = 0; r < R && ok; ++r) { if (lens[(size_t)r]) ok = cm->rccl->recv(dRecv + at, (size_t)lens[(size_t)r], ncclUint8, r, cm->comm, c->stream) == ncclSuccess; at += (size_t)lens[(size_t)r]; }
  }
  ok = (cm->rccl->groupEnd() == ncclSuccess) && ok;
  if (!ok) return fail(c, T4_ERR_HIP, "ncclSend / ncclRecv (gather) failed");
  if (int wr = commWait(cm, "the gather")) return wr;   // (before the copy below: see commLengths)
  if (cm->rank == root) {
    bufs.host = malloc(total ? total : 1);
    if (!bufs.host) return fail(c, T4_ERR_HIP, "out of host memory for the gather");
    if (total) HIPCHK(c, hipMemcpy(bufs.host, dRecv, total, hipMemcpyDeviceToHost));
  }
  *all = bufs.releaseHost();
  return T4_OK;
#else
  return T4_ERR_UNSUPPORTED;
#endif
}

void t4_comm_destroy(t4_comm *cm) {
  if (!cm) return;
#ifdef __HIPCC__
  if (cm->comm) (void)cm->rccl->commDestroy(cm->comm);
#endif
  delete cm;
}

}  // extern "C"
