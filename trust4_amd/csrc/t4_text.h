// trust4_amd/csrc/t4_text.h -- FASTQ text on the device: line table, record validation, 2-bit packing, the low-complexity rule, the
// combine step of the stage-0 candidate test and stage 1's ProcessRead on pairs that lie in two pieces (included by t4_api.hip
// behind t4_kernels.h, namespace t4k).
//
// A piece of text of nbytes bytes lies in device memory padded to a whole number of tiles (T4_TEXT_TILE bytes, one workgroup of
// T4_TEXT_THREADS lanes with one 16-byte load each), so every load is in bounds; bytes at or beyond nbytes never count. Line j of the
// piece is [lineStart[j], lineStart[j + 1] - 1): lineStart[0] = 0, lineStart[j + 1] = one past the j-th '\n'; a last line without its
// '\n' (final piece) ends at nbytes, i.e. its lineStart[j + 1] is nbytes + 1. Record i is lines 4 i .. 4 i + 3.
#pragma once

#define T4_TEXT_THREADS 256
#define T4_TEXT_TILE (T4_TEXT_THREADS * 16)
// per-piece words the kernels leave for the host (unsigned long long each)
#define T4_TEXT_NEWLINES 0   // '\n' bytes of the piece
#define T4_TEXT_BAD 1        // min over the failing records of (record << 4 | status); all ones: none
#define T4_TEXT_LONGEST 2    // longest sequence line among the records looked at
#define T4_TEXT_END 3        // lineStart behind the last record looked at (t4_text_batch of a part: the longest read of the part)
#define T4_TEXT_INFO_WORDS 4

namespace t4k {

// newlines among the 16 bytes this lane loads (bit b of the result: byte b is one); bytes at or beyond nbytes are not looked at
__device__ __forceinline__ unsigned textNewlineBits(const char *text, long long nbytes, long long at) {
  const uint4 v = *(const uint4 *)(text + at);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // byte compare of four bytes at once: a zero byte of x marks a '\n' (exact form: no carries between bytes)
    const unsigned x = w[k] ^ 0x0a0a0a0au;
    const unsigned z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 in every byte of x that is zero
    bits |= ((z >> 7 & 1u) | (z >> 14 & 2u) | (z >> 21 & 4u) | (z >> 28 & 8u)) << (4 * k);
  }
  const long long left = nbytes - at;
  if (left < 16) bits &= left <= 0 ? 0u : (1u << (int)left) - 1u;
  return bits;
}

// sum of v over the workgroup's lanes (T4_TEXT_THREADS lanes, whole waves); s: one word per wave
__device__ __forceinline__ unsigned textBlockSum(unsigned v, unsigned *s) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s[wave] = v;
  __syncthreads();
  unsigned t = 0;
  for (int w = 0; w < T4_TEXT_THREADS / 64; ++w) t += s[w];
  __syncthreads();
  return t;
}

// pass 1: newlines per tile
__global__ __launch_bounds__(T4_TEXT_THREADS) void textCountKernel(const char *text, long long nbytes, unsigned *tileCnt) {
  __shared__ unsigned s_w[T4_TEXT_THREADS / 64];
  const long long at = (long long)blockIdx.x * T4_TEXT_TILE + (long long)threadIdx.x * 16;
  const unsigned total = textBlockSum((unsigned)__popc(textNewlineBits(text, nbytes, at)), s_w);
  if (threadIdx.x == 0) tileCnt[blockIdx.x] = total;
}

// pass 2 (one workgroup): tileCnt becomes its exclusive scan, info receives the piece's newline count
__global__ __launch_bounds__(T4_TEXT_THREADS) void textScanKernel(unsigned *tileCnt, int ntiles, unsigned long long *info) {
  __shared__ unsigned s_sum[T4_TEXT_THREADS];
  const int per = (ntiles + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS;
  const int lo = (int)threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
  unsigned mine = 0;
  for (int t = lo; t < hi; ++t) mine += tileCnt[t];
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  unsigned before = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) before += s_sum[t];
  for (int t = lo; t < hi; ++t) { const unsigned c = tileCnt[t]; tileCnt[t] = before; before += c; }
  if (threadIdx.x == T4_TEXT_THREADS - 1) info[T4_TEXT_NEWLINES] = before;
}

// pass 3: the offsets. tileBase: the scanned tile counts; openEnd: the piece ends in a line without '\n', which ends at nbytes
__global__ __launch_bounds__(T4_TEXT_THREADS) void textFillKernel(const char *text, long long nbytes, const unsigned *tileBase, unsigned *lineStart,
                                                                  int openEnd, const unsigned long long *info) {
  __shared__ unsigned s_w[T4_TEXT_THREADS / 64];
  const long long at = (long long)blockIdx.x * T4_TEXT_TILE + (long long)threadIdx.x * 16;
  unsigned bits = textNewlineBits(text, nbytes, at);
  const unsigned mine = (unsigned)__popc(bits);
  // exclusive scan of the lane counts: inside the wave by shuffles, across the workgroup's waves through LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = mine;
  for (int d = 1; d < 64; d <<= 1) { const unsigned up = __shfl_up(incl, (unsigned)d); if (lane >= d) incl += up; }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  unsigned before = tileBase[blockIdx.x] + incl - mine;
  for (int w = 0; w < wave; ++w) before += s_w[w];
  while (bits) {
    const int b = __ffsll((unsigned long long)bits) - 1;
    bits &= bits - 1;
    lineStart[1 + before++] = (unsigned)(at + b + 1);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    lineStart[0] = 0;
    if (openEnd) lineStart[info[T4_TEXT_NEWLINES] + 1] = (unsigned)(nbytes + 1);
  }
}

// ---- records ---------------------------------------------------------------------------------------------------------------------
// One half-wavefront (32 lanes) per record: records first + i, i < n, of the scanned piece.
// PACK false (t4_text_scan): the checks of the status table (the first failing check of a record gives its status, the
// lowest failing record of the piece is left in info[T4_TEXT_BAD]), and len / low / recStart of every record, info[T4_TEXT_LONGEST].
// PACK true (t4_text_batch, records that passed): row i of the batch -- pk (lane l packs bases 16 l .. 16 l + 15), nm (lanes 2 m and
// 2 m + 1 combine through a shuffle), len, low. Coding of t4_reads_upload_flags with T4_READS_KMERS_ONLY: ACGT 0..3, N mask bit and
// code 0, any other letter 3.
// low = isLowComplexity of FastqExtractor.cpp:105-127: counts of A, C, G, T, N over the letters as written.
template <bool PACK>
__global__ __launch_bounds__(T4_TEXT_THREADS) void textRecordKernel(const char *text, const unsigned *lineStart, long long first, long long n,
                                                                    int *len, unsigned char *low, unsigned *recStart, unsigned long long *info,
                                                                    unsigned *pk, unsigned *nm, int wpk, int wnm) {
  const int l = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
  const long long i = ((long long)blockIdx.x * T4_TEXT_THREADS + threadIdx.x) >> 5;
  const bool live = i < n;   // (a half-wavefront without a record goes through the wave-wide steps with an empty one)
  const long long r = first + (live ? i : 0);
  unsigned s[5];
  for (int k = 0; k < 5; ++k) s[k] = live ? lineStart[4 * r + k] : (unsigned)(k + 1);
  const unsigned seqAt = s[1], qualAt = s[3];
  const int idLen = (int)(s[1] - 1 - s[0]), plusLen = (int)(s[3] - 1 - s[2]);
  const long long seqLen = (long long)s[2] - 1 - s[1], qualLen = (long long)s[4] - 1 - s[3];
  int status = 0;
  if (!PACK && live) {
    if (idLen < 1 || text[s[0]] != '@') status = 1;
    else if (plusLen < 1 || text[s[2]] != '+') status = 2;
    else if (qualLen != seqLen) status = 3;
    else if (seqLen > 0 && (text[seqAt] == '@' || text[seqAt] == '>' || text[seqAt] == '+')) status = 4;
  }
  if (!PACK) {
    // status 5 looks at every byte of the record, however long its lines are (a read beyond T4_MAXL is status 6 only if its bytes are clean)
    int dirty = 0;
    const unsigned end = s[4] - 1;
    for (unsigned p = s[0] + (unsigned)l; live && p < end; p += 32) {
      const unsigned char ch = (unsigned char)text[p];
      const bool body = (p >= seqAt && p < s[2] - 1) || (p >= qualAt && p < end);
      if (ch == '\r' || (body && (ch < 33 || ch > 126))) dirty = 1;
    }
    const unsigned long long b = __ballot(dirty);
    if (status == 0 && ((b >> (32 * half)) & 0xffffffffull)) status = 5;
    if (status == 0 && seqLen > T4_MAXL) status = 6;
  }
  // the lane's 16 bases
  const int ln = live && seqLen <= T4_MAXL ? (int)seqLen : 0;
  unsigned word = 0, mask = 0, cntACG = 0, cntTN = 0;
  int other = 0;
  for (int k = 0; k < 16; ++k) {
    const int j = 16 * l + k;
    if (j >= ln) break;
    const char ch = text[seqAt + j];
    unsigned v = 3;
    if (ch == 'A') { v = 0; cntACG += 1u; }
    else if (ch == 'C') { v = 1; cntACG += 1u << 10; }
    else if (ch == 'G') { v = 2; cntACG += 1u << 20; }
    else if (ch == 'T') cntTN += 1u;
    else if (ch == 'N') { v = 0; mask |= 1u << k; cntTN += 1u << 10; }
    else if (ch < 'A' || ch > 'Z') other = 1;
    word |= v << (2 * k);
  }
  if (PACK) {
    const unsigned hi = __shfl_down(mask, 1u);
    if (live && l < wpk) pk[i * wpk + l] = word;
    if (live && !(l & 1) && (l >> 1) < wnm) nm[i * wnm + (l >> 1)] = mask | hi << 16;
  } else {
    const unsigned long long b7 = __ballot(other);
    if (status == 0 && ((b7 >> (32 * half)) & 0xffffffffull)) status = 7;
  }
  for (int d = 16; d > 0; d >>= 1) { cntACG += __shfl_xor(cntACG, d); cntTN += __shfl_xor(cntTN, d); }   // (sums stay below 2^10 per field: ln <= T4_MAXL)
  if (!live || l != 0) return;
  const int c[5] = {(int)(cntACG & 1023u), (int)(cntACG >> 10 & 1023u), (int)(cntACG >> 20 & 1023u), (int)(cntTN & 1023u), (int)(cntTN >> 10 & 1023u)};
  int isLow = c[0] >= ln / 2 || c[1] >= ln / 2 || c[2] >= ln / 2 || c[3] >= ln / 2 || c[4] >= ln / 10;
  int few = 0;
  for (int k = 0; k < 4; ++k) if (c[k] <= 2) ++few;
  if (few >= 2) isLow = 1;
  if (PACK) { len[i] = ln; low[i] = (unsigned char)isLow; return; }   // (the batch's own rows)
  len[r] = ln; low[r] = (unsigned char)isLow; recStart[r] = s[0];
  if (i == n - 1) info[T4_TEXT_END] = s[4];
  if (status) atomicMin(&info[T4_TEXT_BAD], (unsigned long long)r << 4 | (unsigned long long)status);
  else atomicMax(&info[T4_TEXT_LONGEST], (unsigned long long)ln);
}

// longest of len[0, n) into *out (t4_text_batch of a part of the piece)
__global__ __launch_bounds__(T4_TEXT_THREADS) void textMaxLenKernel(const int *len, long long n, unsigned long long *out) {
  const long long i = (long long)blockIdx.x * T4_TEXT_THREADS + threadIdx.x;
  int v = i < n ? len[i] : 0;
  for (int d = 32; d > 0; d >>= 1) { const int o = __shfl_xor(v, d); if (o > v) v = o; }
  if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(out, (unsigned long long)v);
}

// ---- ProcessRead of pairs that lie in two scanned pieces (t4_text_process_pairs) ---------------------------------------------------
// One pair per wavefront: pair i is record firstA + i of piece A (read 1) and record firstB + i of piece B (read 2), both pieces with
// status 0, so no read is longer than T4_MAXL and every record has as many qualities as bases. The wave stages the pair in LDS as
// processPairKernel does -- the text is read once, byte by byte at whatever alignment the lines have -- and runs that kernel's body
// (processPairStaged). meta[i] = {kind, length of read 1 afterwards, flags, where}: a changed read 1 (flag 16) stands at outR + where
// with its qualities at outQ + where, where is -1 otherwise. Lane 0 takes the room from *need; a read that would reach beyond outCap is
// counted and not written (where -1: the host sees *need > outCap and the call is repeated with more room). skip[i] != 0: the pair
// is not looked at, its kind is -1.
__global__ __launch_bounds__(64) void textProcessPairKernel(const char *textA, const unsigned *lineA, long long firstA, const char *textB, const unsigned *lineB,
                                                            long long firstB, long long n, const unsigned char *skip, char *outR, char *outQ,
                                                            long long outCap, unsigned long long *need, int4 *meta) {
  __shared__ char s_r1[T4_MAXL + 8], s_q1[T4_MAXL + 8], s_f[T4_MAXL + 8], s_fq[T4_MAXL + 8];
  __shared__ char s_m[2 * T4_MAXL + 16], s_mq[2 * T4_MAXL + 16];
  const int lane = laneId();
  for (long long p = blockIdx.x; p < n; p += gridDim.x) {
    if (skip && skip[p]) { if (lane == 0) meta[p] = make_int4(-1, 0, 0, -1); continue; }
    const unsigned *la = lineA + 4 * (firstA + p), *lb = lineB + 4 * (firstB + p);
    const unsigned seqA = la[1], qualA = la[3], seqB = lb[1], qualB = lb[3];
    int slen = (int)(la[2] - 1 - seqA), flen = (int)(lb[2] - 1 - seqB);
    // (what t4_text_scan has checked; held here too, so that no index below leaves the LDS arrays whatever the table says)
    slen = slen < 0 ? 0 : slen > T4_MAXL ? T4_MAXL : slen;
    flen = flen < 0 ? 0 : flen > T4_MAXL ? T4_MAXL : flen;
    for (int i = lane; i < slen; i += 64) { s_r1[i] = textA[seqA + i]; s_q1[i] = textA[qualA + i]; }
    for (int i = lane; i < flen; i += 64) { s_f[i] = rcChar(textB[seqB + flen - 1 - i]); s_fq[i] = textB[qualB + flen - 1 - i]; }
    __syncthreads();
    int kind, outLen, flags;
    processPairStaged(s_r1, s_q1, s_f, s_fq, s_m, s_mq, slen, flen, true, true, kind, outLen, flags);
    int where = -1;
    if (flags & 16) {
      if (lane == 0) {
        const unsigned long long at = atomicAdd(need, (unsigned long long)outLen);
        if (at + (unsigned long long)outLen <= (unsigned long long)outCap && at <= 0x7fffffffull) where = (int)at;
      }
      where = __shfl(where, 0);
      if (where >= 0) for (int j = lane; j < outLen; j += 64) { outR[where + j] = s_m[j]; outQ[where + j] = s_mq[j]; }
    }
    if (lane == 0) meta[p] = make_int4(kind, outLen, flags, where);
    __syncthreads();
  }
}

// ---- the candidate test (FastqExtractor.cpp:129-134, 516-519) ----------------------------------------------------------------------
// Query lengths of one side: 0 for a row that is not to be queried -- a low-complexity read, and a mate whose read passed (done).
__global__ __launch_bounds__(T4_TEXT_THREADS) void candLenKernel(const int *len, const unsigned char *low, const unsigned char *done, int *qlen, long long n) {
  const long long i = (long long)blockIdx.x * T4_TEXT_THREADS + threadIdx.x;
  if (i < n) qlen[i] = ((low && low[i]) || (done && done[i])) ? 0 : len[i];
}
// keep[i] = done[i] || (row i was queried and HasHitInSet != 0)
__global__ __launch_bounds__(T4_TEXT_THREADS) void candCombineKernel(const int *qlen, const int *hit, const unsigned char *done, unsigned char *keep, long long n) {
  const long long i = (long long)blockIdx.x * T4_TEXT_THREADS + threadIdx.x;
  if (i < n) keep[i] = ((done && done[i]) || (qlen[i] > 0 && hit[i] != 0)) ? 1 : 0;
}

}  // namespace t4k
