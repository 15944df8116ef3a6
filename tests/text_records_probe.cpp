// tests/text_records_probe.cpp -- TEST INFRASTRUCTURE ONLY: trust4_amd/host/text_records.h (what trust4-hip's device path cuts its
// read records with) on offset tables made here, under -fsanitize=address,undefined (tests/test_text_records_probe.py). Every piece
// lives in a heap block of exactly its size, so a read one byte outside it is reported. No GPU, no library of the project.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../trust4_amd/host/text_records.h"

namespace {

struct Rec { std::string head, seq, plus, qual; };

int failures = 0;
void expect(bool ok, const char *what, size_t a, size_t b) {
  if (ok) return;
  if (++failures <= 10) fprintf(stderr, "FAILED: %s (%zu, %zu)\n", what, a, b);
}

// where the whole records of text[0, n) begin, as t4_text_scan + t4_text_records give it: a record is four lines; a last line without
// its '\n' counts in a final piece only. The entry behind the last record: where the next one begins (at most n).
std::vector<uint32_t> tableOf(const char *text, size_t n, bool finalPiece) {
  std::vector<size_t> lineStart(1, 0);
  for (size_t i = 0; i < n; ++i) if (text[i] == '\n') lineStart.push_back(i + 1);
  size_t lines = lineStart.size() - 1;
  if (finalPiece && n > 0 && text[n - 1] != '\n') { ++lines; lineStart.push_back(n + 1); }
  std::vector<uint32_t> t;
  const size_t nrec = lines / 4;
  for (size_t r = 0; r <= nrec; ++r) t.push_back((uint32_t)(lineStart[4 * r] < n ? lineStart[4 * r] : n));
  return t;
}

void checkPiece(const std::string &text, size_t cut, bool finalPiece, const std::vector<Rec> &recs) {
  char *piece = (char *)malloc(cut ? cut : 1);   // (exactly the piece: the sanitizer sees every byte beyond it)
  memcpy(piece, text.data(), cut);
  const std::vector<uint32_t> t = tableOf(piece, cut, finalPiece);
  const size_t nrec = t.size() - 1;
  expect(nrec <= recs.size(), "more records than written", nrec, recs.size());
  for (size_t k = 0; k < nrec && k < recs.size(); ++k) {
    t4host::TextRecord r;
    const bool ok = t4host::cutTextRecord(piece, cut, t.data(), k, r);
    expect(ok, "a whole record was not cut", cut, k);
    if (!ok) continue;
    expect(std::string(r.head, r.headLen) == recs[k].head, "header line", cut, k);
    expect(std::string(r.seq, r.seqLen) == recs[k].seq, "sequence", cut, k);
    // (a piece that ends inside the last quality line of an open file holds a prefix of it: only a final piece is cut there)
    const std::string q(r.qual, r.qualLen);
    expect(q == recs[k].qual || (finalPiece && k == nrec - 1 && cut < text.size() && recs[k].qual.compare(0, q.size(), q) == 0), "qualities", cut, k);
    std::string id;
    t4host::textRecordId(r, true, id);
    std::string want = recs[k].head.substr(1, recs[k].head.find_first_of(" \t") == std::string::npos ? std::string::npos : recs[k].head.find_first_of(" \t") - 1);
    if (want.size() >= 2 && want[want.size() - 2] == '/' && (want.back() == '1' || want.back() == '2')) want.resize(want.size() - 2);
    expect(id == want, "id", cut, k);
    t4host::textRecordId(r, false, id);
    expect(id.size() >= want.size(), "id as written", cut, k);
  }
  free(piece);
}

// tables that do not fit the text: nothing may be read outside the piece, and no record may come out of less than four lines
void checkBadTables(const std::string &text) {
  const size_t n = text.size();
  char *piece = (char *)malloc(n);
  memcpy(piece, text.data(), n);
  t4host::TextRecord r;
  const uint32_t beyond[2] = {(uint32_t)n, (uint32_t)(n + 100)};
  expect(!t4host::cutTextRecord(piece, n, beyond, 0, r), "a record that begins at the end", 0, 0);
  const uint32_t far[2] = {(uint32_t)(n + 5), (uint32_t)(n + 50)};
  expect(!t4host::cutTextRecord(piece, n, far, 0, r), "a record beyond the piece", 0, 0);
  const uint32_t back[2] = {20, 10};
  expect(!t4host::cutTextRecord(piece, n, back, 0, r), "offsets that go backwards", 0, 0);
  const uint32_t same[2] = {7, 7};
  expect(!t4host::cutTextRecord(piece, n, same, 0, r), "an empty range", 0, 0);
  const uint32_t all[2] = {0, 0xffffffffu};
  expect(t4host::cutTextRecord(piece, n, all, 0, r) && r.head == piece, "an end beyond the piece is held to it", 0, 0);
  for (size_t lo = 0; lo < n; ++lo)     // every range of the text, whatever it begins and ends in
    for (size_t hi = lo; hi <= n + 1; ++hi) {
      const uint32_t t[2] = {(uint32_t)lo, (uint32_t)hi};
      if (!t4host::cutTextRecord(piece, n, t, 0, r)) continue;
      const size_t end = hi < n ? hi : n;
      expect(r.head == piece + lo && r.seq > r.head && r.qual > r.seq && r.qual + r.qualLen <= piece + end, "a cut record lies inside its range", lo, hi);
      size_t nl = 0;
      for (size_t i = lo; i < end; ++i) nl += piece[i] == '\n';
      expect(nl >= 3, "a record of fewer than four lines", lo, hi);
    }
  free(piece);
}

}  // namespace

int main() {
  const std::vector<Rec> recs = {
      {"@r0", "ACGT", "+", "FFFF"},
      {"@r1/1 a comment", "ACGTNACGTTTGACCA", "+r1/1", "IIIIIIIIIIIIIII#"},
      {"@e", "", "+", ""},                                   // an empty read: "@e\n\n+\n\n"
      {"@r3/2\tx", "A", "+", "!"},
      {"@q/1/2", "GGGGCCCC", "+", "@@@@++++"},               // qualities that look like header and '+' lines
      {"@last", "TTGCA", "+", "~~~~~"},
  };
  for (int openEnd = 0; openEnd < 2; ++openEnd) {
    std::string text;
    for (const Rec &r : recs) text += r.head + "\n" + r.seq + "\n" + r.plus + "\n" + r.qual + "\n";
    if (openEnd) text.pop_back();   // a file whose last line has no '\n'
    for (size_t cut = 0; cut <= text.size(); ++cut) {
      checkPiece(text, cut, false, recs);
      checkPiece(text, cut, true, recs);
    }
    checkBadTables(text);
  }
  if (failures) { printf("FAILED %d checks\n", failures); return 1; }
  printf("ok text records: %zu records, pieces cut at every byte\n", recs.size());
  return 0;
}
