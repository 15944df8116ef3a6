// trust4_amd/csrc/t4_internal.h -- library-internal interface between the host-side contig builder
// (t4_assembler.cpp) and the device side (t4_api.hip). Not part of the public C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/trust4_hip.h"

extern "C" {

// Device arena of per-barcode set images (in barcode mode every cell is an independent SeqSet,
// main.cpp:1556-1559 + SeqSet.hpp:1418). One slot per open cell; a slot's image is rebuilt from the host replica of
// the cell (sequences, posWeight, explicit postings) and uploaded with all other rebuilt images of a window in one
// host-to-device copy + one scatter kernel.
typedef struct t4_cellstore t4_cellstore;
int t4_cellstore_create(t4_ctx *ctx, int kmer_length, t4_cellstore **out);
void t4_cellstore_destroy(t4_cellstore *cs);
int t4_cellstore_set_params(t4_cellstore *cs, int hit_len_required, int radius, double novel_seq_similarity);
int t4_cellstore_open(t4_cellstore *cs, int *slot);
int t4_cellstore_close(t4_cellstore *cs, int slot);
// Queue the new image of one cell. names/cons: nseq C strings ("" for released slots), pw[i]: 4 counts per base of
// sequence i; the index as nkeys lists: key (key_code, key_bucket) owns the next key_cnt (idx, offset) pairs of `post`
// (idx local to the cell, list order = the order KmerIndex holds them in).
int t4_cellstore_stage(t4_cellstore *cs, int slot, int barcode, int nseq, const char *const *names, const char *const *cons,
                       const int32_t *const *pw, int64_t nkeys, const uint64_t *key_code, const int32_t *key_bucket,
                       const int32_t *key_cnt, const int32_t *post, int64_t *pw_offset_in_image,
                       const int32_t *seq_barcodes /* nullable: per-sequence barcodes of a set that is not keyed by barcode */);
// The same image with its table built on the device: staging receives the (code, start, cnt) records of the keys that own
// postings, the image from its postings on and the view -- none of the table's empty slots. The flush writes the table's
// slots empty in the arena and inserts the records there (cellTableBuildKernel); lookups see the same map. The same code
// twice in key_code is refused by the flush (T4_ERR_ARG) and leaves that slot's table incomplete.
int t4_cellstore_stage_compact(t4_cellstore *cs, int slot, int barcode, int nseq, const char *const *names, const char *const *cons,
                               const int32_t *const *pw, int64_t nkeys, const uint64_t *key_code, const int32_t *key_bucket,
                               const int32_t *key_cnt, const int32_t *post, int64_t *pw_offset_in_image, const int32_t *seq_barcodes);
// The same image with its table AND its postings built on the device from the image's own contigs (the indexed form): every posting
// (i, o) of a cell's index has the code of contig i's k-mer at o, so the index travels as one count byte per consensus byte --
// post_cnt[i][o] = the postings (i, o) the index holds; post_cnt_len[i] bytes of contig i are given (post_cnt_len null: as many as
// the contig has bases), a null post_cnt[i] and every byte not given mean zero. Staging receives [count bytes, padded to 16]
// [image from its sequence records on] [view]; the flush runs cellIndexBuildKernel ahead of the scatter. The table has the slots
// of nkeys keys (the image's layout is that of t4_cellstore_stage with nkeys keys and npost postings; everything from the sequence
// records on and the view are byte-equal), so nkeys must be at least the distinct k-mers counted. Every contig carries `barcode`.
// Refused here with T4_ERR_ARG, nothing queued: a count at an offset o with o + k beyond the contig, counts that do not add up to
// npost, npost > 0 with nkeys == 0. Refused by the flush (T4_ERR_ARG naming the slot, which is to be staged again; the other images of
// the flush are whole): a counted offset whose k-mer holds a letter outside ACGT, more distinct k-mers than the table can hold.
int t4_cellstore_stage_indexed(t4_cellstore *cs, int slot, int barcode, int nseq, const char *const *names, const char *const *cons,
                               const int32_t *const *pw, int64_t nkeys, int64_t npost, const uint8_t *const *post_cnt,
                               const int32_t *post_cnt_len, int64_t *pw_offset_in_image);
size_t t4_cellstore_indexed_image_bytes(int nseq, int64_t cons_bytes);   // staged size of one such image, exact
// 4 values: images indexed on the device, count bytes shipped for them (padded), postings written on the device, table bytes
// written on the device (16 per slot). t4_cellstore_image_stats' first three values do not count these images; its fourth does.
int t4_cellstore_indexed_stats(const t4_cellstore *cs, int64_t *out4);
// The resident form: the image stays in its slot between rounds and a change travels as the contigs it touched. The slot keeps
// [table] [postings] [records] and three byte blocks of equal size -- predicate bytes, consensus, count bytes -- in which contig i owns
// one stretch (room for 64 more bases, rounded up to a multiple of 128) that never moves; the table is sized from npost (distinct keys
// <= postings, load <= 2/3, at least 64 slots), the postings have the room that table can serve, there are spare records and spare
// stretch room for contigs to come. The flush runs cellDeltaApplyKernel (touched contigs into their stretches, their records, the view),
// then cellIndexBuildKernel, which rebuilds table and postings from the contigs and counts as they lie in the slot.
// n_touched < 0: the whole image -- names, cons, pw, post_cnt, post_cnt_len have nseq entries, the slot gets a fresh layout.
// n_touched >= 0: a delta -- the arrays have n_touched entries, entry j for contig touched_ids[j] (ascending); a new contig and a
// released one ("") are touched contigs, an untouched contig keeps everything including its counts; npost is the new total.
// post_cnt as for t4_cellstore_stage_indexed. pw_offsets (nullable, nseq values): byte offset of every contig's predicate bytes in
// the image, for t4_cellstore_patch. Returns T4_OK, or T4_CELL_DELTA_WHOLE with nothing queued: the delta does not fit the slot's
// layout (a contig beyond its stretch, more contigs than records or stretch room, more postings than the table serves) and the cell
// is to be staged whole. Refused with T4_ERR_ARG, nothing queued: a touched id out of range or out of order, a new contig that is
// not touched, a count at o + k beyond the contig, counts that do not add up to npost, a delta for a slot without a resident image
// (never staged whole, recycled, or staged in another form since). Refused by the flush as for the indexed form (a counted offset
// whose k-mer has a letter outside ACGT); that slot then holds no resident image.
#define T4_CELL_DELTA_WHOLE 1
int t4_cellstore_stage_delta(t4_cellstore *cs, int slot, int barcode, int nseq, int n_touched, const int32_t *touched_ids,
                             const char *const *names, const char *const *cons, const int32_t *const *pw, const uint8_t *const *post_cnt,
                             const int32_t *post_cnt_len, int64_t npost, int64_t *pw_offsets);
// staged size of n contigs of the given lengths in that form, whole image or delta alike, exact
size_t t4_cellstore_resident_image_bytes(int n, const int32_t *lens);
// 1: t4_cellstore_stage_delta would take this delta (lens[j]: bases of contig touched_ids[j]); 0: the cell is to be staged whole
int t4_cellstore_delta_fits(t4_cellstore *cs, int slot, int nseq, int n_touched, const int32_t *touched_ids, const int32_t *lens, int64_t npost);
#ifdef T4_TEST_KNOBS
// Test builds only: the index of contig seq_idx is built `times` more times over the contig as it stands (every indexed offset gets
// that many more equal postings) -- the only way to more than 255 postings at one offset in a few calls.
int t4_assembler_test_index_again(t4_assembler *a, int seq_idx, int times);
#endif
// 7 values: images staged whole, deltas, contigs shipped by deltas, deltas refused with T4_CELL_DELTA_WHOLE, whole images of slots
// that held a resident image already, postings and table bytes (16 per slot) written on the device for this form
int t4_cellstore_resident_stats(const t4_cellstore *cs, int64_t *out7);
// Overwrite posWeight predicate bytes of the slot's resident image (byte offsets as returned by the last stage + the
// column's index); applied after the staged images of the same flush.
int t4_cellstore_patch(t4_cellstore *cs, int slot, int n, const int64_t *byte_offsets, const unsigned char *values);
// Staged size of one image -- t4_cellstore_image_bytes: by t4_cellstore_stage_compact (exact when every key owns postings,
// an upper bound otherwise); t4_cellstore_full_image_bytes: by t4_cellstore_stage, exact -- and the serial reservation that
// must precede a group of stage calls (which may then run concurrently on several host threads: nothing moves while they write).
size_t t4_cellstore_image_bytes(int nseq, int64_t nkeys, int64_t npost, int64_t cons_bytes);
size_t t4_cellstore_full_image_bytes(int nseq, int64_t nkeys, int64_t npost, int64_t cons_bytes);
int t4_cellstore_prepare(t4_cellstore *cs, int max_slot, size_t bytes);
// Flush the staged images, then run the AddRead query (== t4_add_query) of read i against the image of slot[i].
int t4_cellstore_query(t4_cellstore *cs, int n, const int32_t *slots, const char *bases, const int64_t *offsets,
                       const int32_t *barcodes, const int32_t *strands, int skip_repeats, const double *factors,
                       int max_per_read, int32_t *counts, t4_overlap *ov, t4_overlap *ext, int32_t *ext_ret);
int t4_cellstore_set_big_first(t4_cellstore *cs, int on);   // first launch on the 8192-hit tier (one big set) instead of the 1024-hit tier
int64_t t4_cellstore_bytes_staged(const t4_cellstore *cs);
// 4 values: images whose table was built on the device, key records shipped for them, table bytes written on the device
// (16 per slot), bytes staged over PCIe (== t4_cellstore_bytes_staged)
int t4_cellstore_image_stats(const t4_cellstore *cs, int64_t *out4);
// The host's own count of the keys with postings over all images a t4_cellset has staged: what value 1 of
// t4_cellset_image_stats (key records the device builds were given) must equal.
int64_t t4_cellset_live_keys_staged(const t4_cellset *cs);
// Test and diagnostic aid: flushes, synchronises and copies the slot's image (table first) and its view (128 bytes) to
// the host. *bytes receives the image's size; buf may be null to ask for it.
int t4_cellstore_read_image(t4_cellstore *cs, int slot, void *buf, size_t cap, size_t *bytes, void *view);

// Test aids of the text front end (t4_text.h): the rows of a batch as they lie on the device (dims: words per pk row, words per nm
// row, longest read; low: zeros for a batch that carries no low-complexity bytes; any pointer may be null), the line table of the
// piece last scanned (lines + 1 offsets; *lines alone when line_start is null) and the tile of the line-table kernels.
int t4_batch_read(t4_batch *b, int32_t dims[3], uint32_t *pk, uint32_t *nm, int32_t *len, uint8_t *low);
int t4_text_lines(t4_text *tx, uint32_t *line_start, int64_t cap, int64_t *lines);
int t4_text_tile_bytes(void);
// ... and the qualities a batch of t4_text_pairs_batch carries: *nbytes = how many bytes (-1: the batch carries none, and nothing
// else is written), quals (room for cap >= *nbytes bytes; or null), qual_off (n + 1 offsets; or null)
int t4_batch_quals(t4_batch *b, char *quals, int64_t cap, int64_t *qual_off, int64_t *nbytes);

// t4_add_query with variable-size results (a read may overlap thousands of contigs that share a gene segment): counts[i]
// records of read i start at index base[i] of ov / ext / ext_ret, which point into pinned memory of the ctx that stays
// valid until the next query on it. tier_hint (nullable, n bytes, in/out): nonzero = the read outgrew the LDS tiers the last
// time it was queried, so it starts on the global-scratch tier, beside the launch of the others.
int t4_add_query_pool(t4_index *ix, int n, const char *bases, const int64_t *offsets, const int32_t *barcodes, const int32_t *strands,
                      int skip_repeats, const double *factors, const int32_t **counts, const int32_t **base, const t4_overlap **ov,
                      const t4_overlap **ext, const int32_t **ext_ret, unsigned char *tier_hint);

// the same in two halves, so that the caller's host work overlaps the kernels: begin enqueues, done polls (1 = finished or idle),
// end waits and returns the result. tier_hint must stay alive until end; one call in flight per ctx.
// only_seq (nullable): only_seq[i] >= 0 asks for the overlaps of read i with that one contig alone -- all of them, both strands,
// scored and extended, none of the steps that look across contigs applied (the restricted re-query of a window entry). It reads the
// contig's postings off the posting marks of the image's predicate bytes (t4_device.h T4_PW_MARK_*, written by t4_assembler::makeDelta).
// A read that meets a posting list beyond 10000 entries is answered like any other unless it was armed (t4_add_query_arm_long_lists,
// below): then the two removeOnlyRepeats tests of GetOverlapsFromHits (SeqSet.hpp:871-887, 931-947) are applied to the contig's two
// groups from the flags and the head of the read's last whole query (t4_add_query_head) and the list sizes of this call's own seed
// stage, a run that ends beyond the head is refused (status 5: ask for the whole query), and the call reports what the statistics
// loop reads of the contig's two groups for removeOnlyRepeats (t4_add_query_last_long_lists).
// The candidate store: with want_cands the call also returns, per read, EVERY scored overlap of the pass on the strand of
// the best one as it stands before the similarity cut (a restricted re-query: every overlap with its one contig) in the order of the
// scan of SeqSet.hpp:1673-2094 -- pre-score key, scored fields, whether the pre-filters of 1705-1794 cut it -- and eight statistics
// words per read: per strand (minus, plus) the groups of >= 4 hits, of >= 5 hits, the largest group (true sizes; a restricted
// re-query: of its one contig) and the novelMinHitRequired the pass used (SeqSet.hpp:784-823); a restricted re-query adds the hull of
// the read's projections along the contig's diagonals with three or more hits (lo minus / plus, hi minus / plus; lo > hi: none):
// T4_QUERY_STATS words per read. want_cands: 1 = return the candidate records. force_min (nullable, restricted re-queries): that
// threshold for the one contig's groups, minus | plus << 16 (0: three hits).
#define T4_QUERY_STATS 12
typedef struct { int32_t seqIdx, ss, se; int16_t rs, re, m0, matchCnt, indelCnt; uint16_t flags; } t4_cand;   // flags: 1 plus strand, 2 scoring left similarity 0, 4 cut by the pre-filters
int t4_add_query_pool_begin2(t4_index *ix, int n, const char *bases, const int64_t *offsets, const int32_t *barcodes, const int32_t *strands,
                             int skip_repeats, const double *factors, unsigned char *tier_hint, const int32_t *only_seq, const int32_t *force_min, int want_cands);
int t4_add_query_last_cands(t4_ctx *ctx, const t4_cand **pool, const int32_t **base, const int32_t **cnt, const int32_t **stats8, int *n);
int t4_add_query_last_aux(t4_ctx *ctx, const int32_t **aux, const int32_t **n4, const int32_t **status, int *n);   // see T4QueryArgs::aux / n4
int t4_add_query_pool_done(t4_ctx *ctx);
int t4_ctx_device(t4_ctx *ctx);   // the device ordinal the ctx was created on (t4_assembler opens further ctxs beside it: one per query lane)
int t4_add_query_pool_end(t4_ctx *ctx, const int32_t **counts, const int32_t **base, const t4_overlap **ov, const t4_overlap **ext, const int32_t **ext_ret);

// AddRead query path of this ctx, 7 values: calls, reads, launches of the global-scratch tier, reads it served, result records,
// microseconds of its kernels (HIP events on the ctx's stream), _hit records its seed stages emitted
int t4_add_query_stats(t4_ctx *ctx, int64_t *out7);
int t4_add_query_last_stable(t4_ctx *ctx, const int32_t **flags, int *n);   // see T4QueryArgs::statsStable
// the wide query (csrc/t4_wide.h): dependency records of a read it served -- see t4_api.hip
typedef struct { uint32_t key, cnt; int32_t lo, hi; } t4_grp;   // key = contig * 2 + (strand == 1); hits (bits 0-23); hull of the diagonals with three or more hits (lo > hi: none)
// (records of a read with lists beyond 10000 postings -- `huge` -- carry in bits 24-27 of cnt what SeqSet.hpp:796-806 reads of the group:
// bits 24-26 its hits of lists of at most 10000 postings, capped at 4; bit 27 whether its hit lowest on the read is one)
int t4_add_query_groups(t4_ctx *ctx, int i, const t4_grp **groups, int *n, int *huge, int *n4);
// the head of a `huge` read the wide query served: 1 with M, the first M entries of the read's hit array in the reference's order
// (strand, contig, read offset) as a bitmap (1 = list of at most 10000 postings; pinned memory, valid until the next call) and
// removeOnlyRepeats (minus | plus << 1); 0 for every other read -- nothing is kept for those
int t4_add_query_head(t4_ctx *ctx, int i, int *m, const uint32_t **bits, int *ror);
// arms the restricted re-queries of the NEXT t4_add_query_pool_begin2 call on the ctx (n reads, with only_seq): arm[i] = ror minus |
// ror plus << 1 | 4 | M << 3 as t4_add_query_head gave them (0: not armed -- the plain restricted path), head_word[i] = first word
// of the read's bitmap in heads[0, n_words) (copied)
int t4_add_query_arm_long_lists(t4_ctx *ctx, int n, const int32_t *arm, const int32_t *head_word, const uint32_t *heads, int n_words);
// per read of the last call, null when it was not armed: 0x100 | bits 24-27 of t4_grp::cnt as the one contig's minus group would
// carry them | the plus group's << 4 (armed re-queries that were answered; 0 otherwise)
int t4_add_query_last_long_lists(t4_ctx *ctx, const int32_t **info, int *n);
int t4_add_query_wide_stats(t4_ctx *ctx, int64_t *out4);
int t4_add_query_defer_stats(t4_ctx *ctx, int64_t *out1);
int t4_add_query_last_call(t4_ctx *ctx, double *kernel_ms, const int32_t **ticks10ns, int *n);   // development aid (T4_ROUND_LOG)
// AssignRead's pick over caller-supplied records (assignPickKernel as t4_assign_wide runs it, one workgroup per read): counts[i] records of
// read i (lens[i] bases) start at base[i] of ov (GetOverlapsFromRead's), ext / ret (ExtendOverlap's result and return value) and aux
// (0: the extension failed the similarity cut, else the denominator of its similarity), n_rec records each. For the tests of the
// pick: contig sets leave indelCnt 0 in every overlap GetOverlapsFromRead returns, so the field AssignRead leaves behind after a
// similarity-failed extension is only seen to move with records made by hand.
int t4_assign_pick(t4_ctx *ctx, int n_reads, const int32_t *counts, const int32_t *base, const int32_t *lens, int64_t n_rec, const t4_overlap *ov,
                   const t4_overlap *ext, const int32_t *ret, const int32_t *aux, int32_t *out_ret, t4_overlap *out);

}  // extern "C"
