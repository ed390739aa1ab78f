// mh_piecequeue.h — the queue between a producer of ready pieces of a device buffer and the one thread that copies them
// out (BgzfSink, mh_bgzfsink.hip).  The consumer takes the pieces in push order, cut front to back into sub-pieces of
// at most slot_bytes, and reports each piece once its last byte has left the device; the producer can wait for that
// before it overwrites the piece's bytes (the spilled BAM store's two-slot ring, filter-bam's one output buffer).
// Plain C++17, no HIP: tests/sanitize/san_piecequeue.cpp runs it alone.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

namespace mh {

class PieceQueue {
 public:
  struct Sub {
    int64_t off, len;   // 0 < len <= slot_bytes
    void *token;        // the piece's
    int64_t ends;       // the piece whose last bytes these are, or -1
  };

  explicit PieceQueue(int64_t slot_bytes) : slot_(slot_bytes) {}

  // the state a new file starts from (no thread is inside the queue)
  void reset() {
    pieces_.clear();
    item_ = 0;
    in_item_ = 0;
    out_ = 0;
    closed_ = stopped_ = false;
  }

  // ---- producer ----
  // a piece of `bytes` bytes at `off` (0 bytes: nothing to copy; it counts as copied once the pieces before it are)
  void push(int64_t off, int64_t bytes, void *token) {
    std::lock_guard<std::mutex> lk(mu_);
    pieces_.push_back(Piece{off, bytes, token});
    skip_empty();
    cv_.notify_all();
  }
  // the number of pieces pushed so far
  int64_t mark() {
    std::lock_guard<std::mutex> lk(mu_);
    return (int64_t)pieces_.size();
  }
  // waits until every piece before `mark` has left the device; false when the consumer stopped before that
  bool wait_copied(int64_t mark) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return out_ >= mark || stopped_; });
    return out_ >= mark;
  }
  // no more pieces will come
  void close() {
    std::lock_guard<std::mutex> lk(mu_);
    closed_ = true;
    cv_.notify_all();
  }

  // ---- consumer ----
  // waits for the next sub-piece; false once the queue is closed and drained, or stopped (wait false: also when none
  // is ready now)
  bool take(Sub *sub, bool wait = true) {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      while (item_ < pieces_.size() && in_item_ >= pieces_[item_].len) {
        item_++;
        in_item_ = 0;
      }
      if (stopped_) return false;
      if (item_ < pieces_.size()) break;
      if (closed_ || !wait) return false;
      cv_.wait(lk);
    }
    const Piece &p = pieces_[item_];
    sub->off = p.off + in_item_;
    sub->len = p.len - in_item_ < slot_ ? p.len - in_item_ : slot_;
    sub->token = p.token;
    in_item_ += sub->len;
    sub->ends = in_item_ >= p.len ? (int64_t)item_ : -1;
    return true;
  }
  // piece i's last bytes (and so every earlier piece's) have left the device
  void copied(int64_t i) {
    std::lock_guard<std::mutex> lk(mu_);
    if (out_ < i + 1) out_ = i + 1;
    skip_empty();
    cv_.notify_all();
  }
  // the consumer gives up or is done: every waiter wakes
  void stop() {
    std::lock_guard<std::mutex> lk(mu_);
    stopped_ = true;
    cv_.notify_all();
  }

 private:
  struct Piece {
    int64_t off, len;
    void *token;
  };
  void skip_empty() {
    while (out_ < (int64_t)pieces_.size() && pieces_[(size_t)out_].len <= 0) out_++;
  }

  const int64_t slot_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Piece> pieces_;
  size_t item_ = 0;        // the piece being cut
  int64_t in_item_ = 0;    // its bytes already taken
  int64_t out_ = 0;        // pieces [0, out_) have left the device
  bool closed_ = false, stopped_ = false;
};

}  // namespace mh
