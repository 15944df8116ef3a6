// trust4_amd/host/text_records.h -- records cut out of a piece of FASTQ text by the offsets the device found (t4_text_records): what
// trust4-hip's device path (T4_GPU_PARSE=1) builds its read records from. No GPU calls here: tests/text_records_probe.cpp runs this
// code under the sanitizers on offset tables of its own.
//
// recStart[k] is where record k begins in the piece, recStart[k + 1] where the next one begins (for the last record of a final
// piece: the piece's end, with or without a '\n' in front of it). A record is four lines: header, sequence, '+' line, qualities.
// The device has validated the piece (status 0) before anything here runs; all the same nothing below reads outside
// [recStart[k], min(recStart[k + 1], pieceBytes)), whatever the table and the text hold, and a record that does not have its four
// lines in there is reported, not cut.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "seq_reader.h"

namespace t4host {

struct TextRecord {
  const char *head = nullptr, *seq = nullptr, *qual = nullptr;   // into the piece; not terminated
  size_t headLen = 0, seqLen = 0, qualLen = 0;                    // the lines without their '\n'
};

// record k of the piece -> its header line, sequence and qualities in place. false: the table or the text does not hold four lines there.
inline bool cutTextRecord(const char *piece, size_t pieceBytes, const uint32_t *recStart, size_t k, TextRecord &r) {
  const size_t lo = recStart[k], hi = recStart[k + 1] < pieceBytes ? recStart[k + 1] : pieceBytes;
  if (lo >= hi) return false;
  const char *p = piece + lo, *end = piece + hi;
  const char *line[4];
  size_t len[4];
  for (int j = 0; j < 4; ++j) {
    if (p > end || (p == end && j < 3)) return false;   // (an empty last line without its '\n' is a line: "@id\n\n+\n" ends an open piece)
    const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
    if (!nl) {
      if (j < 3) return false;
      nl = end;
    }
    line[j] = p; len[j] = (size_t)(nl - p);
    p = nl + 1;
  }
  r.head = line[0]; r.headLen = len[0];
  r.seq = line[1]; r.seqLen = len[1];
  r.qual = line[3]; r.qualLen = len[3];
  return true;
}

// the record's name as the readers give it (splitHeader: up to the first blank, a trailing /1 or /2 dropped)
inline void textRecordId(const TextRecord &r, bool stripMateSuffix, std::string &id) {
  if (r.headLen == 0) { id.clear(); return; }
  splitHeader(r.head, r.headLen, stripMateSuffix, id, nullptr);
}

}  // namespace t4host
