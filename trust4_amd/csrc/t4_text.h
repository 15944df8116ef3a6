// trust4_amd/csrc/t4_text.h -- FASTQ text on the device: line table, record validation, 2-bit packing, the low-complexity rule, the
// combine step of the stage-0 candidate test, stage 1's ProcessRead on pairs that lie in two pieces and those pairs afterwards as the
// rows of a batch with their qualities (included by t4_api.hip behind t4_kernels.h, namespace t4k).
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

// ---- the pairs after ProcessRead as the rows of a batch (t4_text_pairs_batch) --------------------------------------------------------
// What the driver appends to its read list for pair i (meta[i] of the last t4_text_process_pairs call): read 1 if flag 1 is set, the
// same read once more if flag 4 is set too (a merged read counts twice), read 2 if flag 2 is set; a skipped pair (kind -1, flags 0)
// gives nothing. Rows stand in that order, pairs in input order; the qualities of row r stand at qoff[r] of one byte buffer.
// Three kernels: the rows and bases of every pair with their exclusive scan inside a workgroup of T4_TEXT_THREADS pairs
// (textPairRowsKernel), the scan over the workgroups' sums (textPairScanKernel, one workgroup: the two levels of textCountKernel /
// textScanKernel), and the packing (textPairPackKernel). Words they leave for the host:
#define T4_PAIRROWS_ROWS 0      // rows of the batch
#define T4_PAIRROWS_BASES 1     // bases (= quality bytes) of all rows
#define T4_PAIRROWS_LONGEST 2   // longest row
#define T4_PAIRROWS_OTHER 3     // 1: a surviving read 1 holds a letter other than A, C, G, T, N (it is packed as code 3)
#define T4_PAIRROWS_WORDS 4

// exclusive scan of v over the workgroup's lanes, the sum of all of them in total; s: one word per wave
__device__ __forceinline__ unsigned textBlockExclusive(unsigned v, unsigned *s, unsigned &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = v;
  for (int d = 1; d < 64; d <<= 1) { const unsigned up = __shfl_up(incl, (unsigned)d); if (lane >= d) incl += up; }
  if (lane == 63) s[wave] = incl;
  __syncthreads();
  unsigned before = incl - v;
  total = 0;
  for (int w = 0; w < T4_TEXT_THREADS / 64; ++w) { if (w < wave) before += s[w]; total += s[w]; }
  __syncthreads();
  return before;
}

// length of read 2 of a pair as the line table of piece B has it, held to what t4_text_scan has checked
__device__ __forceinline__ int textMateLen(const unsigned *lb) {
  const long long len = (long long)lb[2] - 1 - (long long)lb[1];
  return len < 0 ? 0 : len > T4_MAXL ? T4_MAXL : (int)len;
}

// One pair per lane. rowAt[p] = {rows, bases} of the pairs ahead of p in its workgroup; blockRows / blockBases[workgroup] = its sums.
__global__ __launch_bounds__(T4_TEXT_THREADS) void textPairRowsKernel(const int4 *meta, const unsigned *lineB, long long firstB, long long n, uint2 *rowAt,
                                                                      unsigned long long *blockRows, unsigned long long *blockBases, unsigned long long *info) {
  __shared__ unsigned s_w[T4_TEXT_THREADS / 64];
  const long long p = (long long)blockIdx.x * T4_TEXT_THREADS + threadIdx.x;
  unsigned rows = 0, bases = 0;
  int longest = 0;
  if (p < n) {
    const int4 m = meta[p];
    const int len1 = m.y < 0 ? 0 : m.y, len2 = textMateLen(lineB + 4 * (firstB + p));
    const unsigned rows1 = (m.z & 1) ? ((m.z & 4) ? 2u : 1u) : 0u, rows2 = (m.z & 2) ? 1u : 0u;
    rows = rows1 + rows2;
    bases = rows1 * (unsigned)len1 + rows2 * (unsigned)len2;   // (a merged read has at most 2 T4_MAXL bases: no carry)
    longest = rows1 ? len1 : 0;
    if (rows2 && len2 > longest) longest = len2;
  }
  unsigned allRows, allBases;
  const unsigned rowsBefore = textBlockExclusive(rows, s_w, allRows), basesBefore = textBlockExclusive(bases, s_w, allBases);
  if (p < n) { uint2 at; at.x = rowsBefore; at.y = basesBefore; rowAt[p] = at; }
  if (threadIdx.x == 0) { blockRows[blockIdx.x] = allRows; blockBases[blockIdx.x] = allBases; }
  for (int d = 32; d > 0; d >>= 1) { const int o = __shfl_xor(longest, d); if (o > longest) longest = o; }
  if ((threadIdx.x & 63) == 0 && longest > 0) atomicMax(&info[T4_PAIRROWS_LONGEST], (unsigned long long)longest);
}

// (one workgroup) the workgroups' sums become their exclusive scans (64-bit: the offsets kmerStatsKernel reads), info receives the totals
__global__ __launch_bounds__(T4_TEXT_THREADS) void textPairScanKernel(unsigned long long *blockRows, unsigned long long *blockBases, int nblocks, unsigned long long *info) {
  __shared__ unsigned long long s_rows[T4_TEXT_THREADS], s_bases[T4_TEXT_THREADS];
  const int per = (nblocks + T4_TEXT_THREADS - 1) / T4_TEXT_THREADS;
  const int lo = (int)threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
  unsigned long long rows = 0, bases = 0;
  for (int t = lo; t < hi; ++t) { rows += blockRows[t]; bases += blockBases[t]; }
  s_rows[threadIdx.x] = rows; s_bases[threadIdx.x] = bases;
  __syncthreads();
  unsigned long long rowsBefore = 0, basesBefore = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) { rowsBefore += s_rows[t]; basesBefore += s_bases[t]; }
  for (int t = lo; t < hi; ++t) {
    const unsigned long long r = blockRows[t], b = blockBases[t];
    blockRows[t] = rowsBefore; blockBases[t] = basesBefore;
    rowsBefore += r; basesBefore += b;
  }
  if (threadIdx.x == T4_TEXT_THREADS - 1) { info[T4_PAIRROWS_ROWS] = rowsBefore; info[T4_PAIRROWS_BASES] = basesBefore; }
}

// One half-wavefront per pair, as textRecordKernel<true> packs: lane l packs bases 16 l .. 16 l + 15 of a row (no row is longer than
// T4_MAXL: the host has looked at info[T4_PAIRROWS_LONGEST]), lanes 2 m and 2 m + 1 combine their N masks through a shuffle. Read 1
// comes from its record, or from pairR + where when flag 16 is set (qualities: pairQ + where); read 2 from its record with every
// letter other than A, C, G, T turned into N. Every byte is read once, at whatever alignment the lines have. qual / qoff null: a
// batch without qualities. A half-wavefront without a row goes through the wave-wide steps with an empty one.
__global__ __launch_bounds__(T4_TEXT_THREADS) void textPairPackKernel(const char *textA, const unsigned *lineA, long long firstA, const char *textB, const unsigned *lineB,
                                                                      long long firstB, long long n, const int4 *meta, const char *pairR, const char *pairQ,
                                                                      long long pairCap, const uint2 *rowAt, const unsigned long long *blockRows,
                                                                      const unsigned long long *blockBases, unsigned *pk, unsigned *nm, int wpk, int wnm, int *len,
                                                                      char *qual, long long *qoff, unsigned long long *info) {
  const int l = threadIdx.x & 31;
  const long long p = ((long long)blockIdx.x * T4_TEXT_THREADS + threadIdx.x) >> 5;
  const bool live = p < n;
  int4 m; m.x = -1; m.y = 0; m.z = 0; m.w = -1;
  long long row = 0, qat = 0;
  unsigned seqA = 0, qualA = 0, seqB = 0, qualB = 0;
  int len2 = 0;
  if (live) {
    m = meta[p];
    const uint2 at = rowAt[p];
    row = (long long)blockRows[p / T4_TEXT_THREADS] + at.x; qat = (long long)blockBases[p / T4_TEXT_THREADS] + at.y;
    const unsigned *la = lineA + 4 * (firstA + p), *lb = lineB + 4 * (firstB + p);
    seqA = la[1]; qualA = la[3]; seqB = lb[1]; qualB = lb[3];
    len2 = textMateLen(lb);
  }
  const int fl = m.z;
  int otherIn1 = 0;
  for (int side = 0; side < 2; ++side) {
    const bool use = (fl & (side ? 2 : 1)) != 0;
    const char *src = textB + seqB, *qsrc = textB + qualB;
    int ln = len2;
    if (side == 0) {
      ln = m.y;
      src = textA + seqA; qsrc = textA + qualA;
      if (fl & 16) {
        // (a call that succeeded has written every changed read inside the buffers; held here too, so that no load leaves them)
        if (m.w < 0 || (long long)m.w + ln > pairCap) ln = 0;
        else { src = pairR + m.w; qsrc = pairQ + m.w; }
      }
    }
    if (!use || ln < 0 || ln > T4_MAXL) ln = 0;
    unsigned word = 0, mask = 0;
    for (int k = 0; k < 16; ++k) {
      const int j = 16 * l + k;
      if (j >= ln) break;
      const char ch = src[j];
      unsigned v = 3;
      if (ch == 'A') v = 0;
      else if (ch == 'C') v = 1;
      else if (ch == 'G') v = 2;
      else if (ch == 'T') v = 3;
      else if (ch == 'N' || side == 1) { v = 0; mask |= 1u << k; }
      else otherIn1 = 1;
      word |= v << (2 * k);
    }
    const unsigned hi = __shfl_down(mask, 1u);
    if (!use) continue;   // (uniform over the half-wavefront; nothing wave-wide below)
    const int copies = side == 0 && (fl & 4) ? 2 : 1;
    if (qual) for (int j = l; j < ln; j += 32) { const char q = qsrc[j]; qual[qat + j] = q; if (copies == 2) qual[qat + ln + j] = q; }
    for (int c = 0; c < copies; ++c) {
      if (l < wpk) pk[row * wpk + l] = word;
      if (!(l & 1) && (l >> 1) < wnm) nm[row * wnm + (l >> 1)] = mask | hi << 16;
      if (l == 0) { len[row] = ln; if (qoff) qoff[row] = qat; }
      ++row; qat += ln;
    }
  }
  if (otherIn1) info[T4_PAIRROWS_OTHER] = 1ull;
  if (live && p == n - 1 && l == 0 && qoff) qoff[info[T4_PAIRROWS_ROWS]] = (long long)info[T4_PAIRROWS_BASES];
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
