// san_piecequeue — stand-alone driver for the piece queue between the device deflate and the thread that copies its
// output to a file (mitty_amd/csrc/mh_piecequeue.h), built by tests/test_host_cpu.py with -fsanitize=address,undefined
// and, where the machine links it, -fsanitize=thread.  Slots of 64 bytes, a producer and a consumer thread.  Prints
// "ok" and exits 0; a broken property is "FAIL <line>: <what>" and exit 1, a deadlock the caller's timeout.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "../../mitty_amd/csrc/mh_piecequeue.h"

using mh::PieceQueue;

#define CHECK(c)                                        \
  do {                                                  \
    if (!(c)) {                                         \
      fprintf(stderr, "FAIL %d: %s\n", __LINE__, #c);   \
      exit(1);                                          \
    }                                                   \
  } while (0)

constexpr int64_t SLOT = 64;

static void *token_of(size_t i) { return (void *)(uintptr_t)(i + 1); }

// pieces of `sizes` at running offsets: the sub-pieces of each are contiguous, in order, at most SLOT bytes, cover it
// exactly, and exactly the last one ends it; a 0-byte piece yields none, yet wait_copied past it returns
static void cut_and_cover(const std::vector<int64_t> &sizes) {
  PieceQueue q(SLOT);
  std::vector<int64_t> offs;
  std::vector<PieceQueue::Sub> subs;
  std::thread consumer([&] {
    PieceQueue::Sub s;
    while (q.take(&s)) {
      subs.push_back(s);
      if (s.ends >= 0) q.copied(s.ends);
    }
    q.stop();
  });
  std::thread producer([&] {
    int64_t o = 1000;
    for (size_t i = 0; i < sizes.size(); i++) {
      offs.push_back(o);
      q.push(o, sizes[i], token_of(i));
      CHECK(q.mark() == (int64_t)i + 1);
      o += sizes[i];
    }
    CHECK(q.wait_copied(0));
    for (size_t i = 0; i < sizes.size(); i++) CHECK(q.wait_copied((int64_t)i + 1));
    q.close();
  });
  producer.join();
  consumer.join();
  size_t k = 0;
  for (size_t i = 0; i < sizes.size(); i++) {
    int64_t at = offs[i];
    const int64_t end = offs[i] + sizes[i];
    while (at < end) {
      CHECK(k < subs.size());
      const PieceQueue::Sub &s = subs[k++];
      CHECK(s.off == at && s.len > 0 && s.len <= SLOT && s.off + s.len <= end);
      CHECK(s.token == token_of(i));
      CHECK(s.len == SLOT || s.off + s.len == end);   // (cut front to back: only the last one is short)
      at += s.len;
      CHECK(s.ends == (at == end ? (int64_t)i : -1));
    }
  }
  CHECK(k == subs.size());
}

// a producer that keeps two windows in flight never pushes window i before the consumer has reported every piece of
// window i - 2 copied
static void two_windows_in_flight() {
  PieceQueue q(SLOT);
  std::mutex mu;            // the test's own
  int64_t reported = 0;     // pieces the consumer has reported copied (set before the report)
  std::thread consumer([&] {
    PieceQueue::Sub s;
    while (q.take(&s)) {
      if (s.ends < 0) continue;
      {
        std::lock_guard<std::mutex> lk(mu);
        reported = s.ends + 1;
      }
      q.copied(s.ends);
    }
    q.stop();
  });
  std::thread producer([&] {
    std::vector<int64_t> marks, need;   // per window: the pieces before its end; ... up to its last piece with bytes
    int64_t o = 0, last = 0;
    for (int i = 0; i < 50; i++) {
      if (i >= 2) {
        CHECK(q.wait_copied(marks[i - 2]));
        std::lock_guard<std::mutex> lk(mu);
        CHECK(reported >= need[i - 2]);
      }
      const int n = 1 + i % 3;
      for (int p = 0; p < n; p++) {
        const int64_t b = (int64_t)((i * 37 + p * 101) % 200);   // 0 .. 199: empty, short and cut pieces
        q.push(o, b, nullptr);
        o += b;
        if (b > 0) last = q.mark();   // (an empty piece is never reported: it is copied once those before it are)
      }
      marks.push_back(q.mark());
      need.push_back(last);
    }
    CHECK(q.wait_copied(marks.back()));
    q.close();
  });
  producer.join();
  consumer.join();
  CHECK(reported <= q.mark());
}

static void close_on_empty() {
  PieceQueue q(SLOT);
  PieceQueue::Sub s;
  CHECK(!q.take(&s, false));   // (nothing ready: no wait when told not to)
  q.push(3, 2, nullptr);
  CHECK(q.take(&s, false) && s.off == 3 && s.len == 2 && s.ends == 0);
  q.reset();
  q.close();
  CHECK(!q.take(&s));
  CHECK(q.wait_copied(0) && q.mark() == 0);
}

// the consumer stops after its second sub-piece: a producer waiting in wait_copied returns false, a later push returns
static void consumer_stops() {
  PieceQueue q(SLOT);
  std::atomic<bool> waiting{false};
  std::thread producer([&] {
    for (int i = 0; i < 3; i++) q.push(64 * i, 64, nullptr);
    waiting = true;
    CHECK(!q.wait_copied(3));
    q.push(192, 64, nullptr);
    CHECK(q.mark() == 4);
    CHECK(!q.wait_copied(4));
    q.close();
  });
  std::thread consumer([&] {
    PieceQueue::Sub s;
    for (int k = 0; k < 2; k++) {
      CHECK(q.take(&s) && s.ends == k);
      if (k == 0) q.copied(s.ends);
    }
    while (!waiting) std::this_thread::yield();
    q.stop();
    CHECK(!q.take(&s));
  });
  producer.join();
  consumer.join();
  CHECK(q.wait_copied(1));   // (what was reported stays reported)
}

int main() {
  cut_and_cover({0, 1, 63, 64, 65, 3 * 64 + 7});
  cut_and_cover({5, 0, 0, 128, 0});   // empty pieces between and behind the others
  cut_and_cover({0});
  two_windows_in_flight();
  close_on_empty();
  consumer_stops();
  // a queue used again for the next file
  {
    PieceQueue q(SLOT);
    q.push(0, 10, nullptr);
    q.stop();
    q.reset();
    q.push(7, 65, nullptr);
    q.close();
    PieceQueue::Sub s;
    CHECK(q.take(&s) && s.off == 7 && s.len == 64 && s.ends == -1);
    CHECK(q.take(&s) && s.off == 71 && s.len == 1 && s.ends == 0);
    CHECK(!q.take(&s));
  }
  printf("ok\n");
  return 0;
}
