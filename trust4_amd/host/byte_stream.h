// trust4_amd/host/byte_stream.h -- the raw bytes of an input file read ahead on a thread of its own: what the device paths of the
// drivers (T4_GPU_PARSE=1; fastq_extractor_main.cpp, trust4_main.cpp) cut their pieces of text from.
#pragma once
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// The raw bytes of one input file (inflated when it is gzip: gzread yields the same bytes) read ahead on a thread of its own in
// chunks, for the device path (T4_GPU_PARSE=1): the main thread takes them into its current piece while the last one is on the device.
struct ByteStream {
  static constexpr size_t DEPTH = 4;
  std::string path;
  size_t chunkBytes = 0;
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::deque<std::vector<char>> q;
  size_t at = 0;   // bytes of q.front() already taken
  bool done = false, stop = false, failed = false;
  void start(const std::string &file, size_t chunk) {
    path = file; chunkBytes = chunk ? chunk : 1;
    th = std::thread([this]() {
      FILE *raw = nullptr;
      gzFile gz = nullptr;
      struct stat st;
      if (stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode) && (raw = fopen(path.c_str(), "rb"))) {   // (as SeqReader::openNext tells the two apart)
        unsigned char magic[2] = {0, 0};
        const size_t got = fread(magic, 1, 2, raw);
        if ((got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) || fseek(raw, 0, SEEK_SET) != 0) { fclose(raw); raw = nullptr; }
      }
      if (!raw && (gz = gzopen(path.c_str(), "rb"))) gzbuffer(gz, 1 << 20);
      bool bad = !raw && !gz;
      for (; !bad;) {
        std::vector<char> v(chunkBytes);
        size_t got = 0;
        if (raw) got = fread(v.data(), 1, v.size(), raw);
        else { const int r = gzread(gz, v.data(), (unsigned)v.size()); if (r < 0) { bad = true; break; } got = (size_t)r; }
        v.resize(got);
        std::unique_lock<std::mutex> lk(m);
        if (got) q.push_back(std::move(v));
        if (got < chunkBytes) break;
        cv.notify_all();
        cv.wait(lk, [this]() { return q.size() < DEPTH || stop; });
        if (stop) break;
      }
      if (raw) fclose(raw);
      if (gz) gzclose(gz);
      std::lock_guard<std::mutex> lk(m);
      failed = bad; done = true;
      cv.notify_all();
    });
  }
  // up to `want` bytes to dst; fewer only at the end of the file. *ended: nothing is left behind them.
  size_t take(char *dst, size_t want, bool *ended) {
    size_t got = 0;
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
      cv.wait(lk, [this]() { return !q.empty() || done; });
      if (q.empty()) { *ended = true; return got; }
      if (got == want) { *ended = false; return got; }
      std::vector<char> &f = q.front();
      const size_t k = std::min(want - got, f.size() - at);
      memcpy(dst + got, f.data() + at, k);
      got += k; at += k;
      if (at == f.size()) { q.pop_front(); at = 0; cv.notify_all(); }
    }
  }
  void finish() {
    if (!th.joinable()) return;
    { std::lock_guard<std::mutex> lk(m); stop = true; }
    cv.notify_all();
    th.join();
  }
};
