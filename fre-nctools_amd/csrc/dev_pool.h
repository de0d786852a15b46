// dev_pool.h -- the caching pool of device blocks behind every plan (plan.hip) and fg_dev_alloc.
//
// Blocks are cached per (device, size class) and never split.  A block can come back in two ways:
//   put(p)          the caller has synchronised: nothing on the device uses the block any more (an UNTAGGED block);
//   put(ps, stream, seal)  work queued on `stream` may still use the blocks (TAGGED blocks).  The blocks of one call form a batch
//                   that shares one ordering-only event.
// and be taken in two ways:
//   get(dev, n, stream)  the block will be used by work queued on `stream` only.  A block tagged with the same stream is handed
//                   out as it is (stream order does the rest); a block tagged with another stream after the stream has been
//                   made to wait for its batch's event on the device, or when the event has passed.  Never a host wait, and
//                   never a fresh allocation while a cached block of the class exists.
//   get(dev, n)     for every other caller: untagged blocks first, then blocks whose event has passed, then a HOST wait for a
//                   tagged one; only an empty class allocates.  Such a caller never sees a block that is still in use, and the
//                   footprint does not grow because tagged blocks were passed over.
// When a batch's event is recorded.  An event recorded later stands behind everything queued on the stream until then, which
// includes the work the batch was tagged for: a later record orders no less, and one record can serve every batch of its stream
// that has none yet.  So a batch put with seal = false waits for its event until somebody needs it (a get from another stream or
// without one, release_all) or until seal(stream) / a put with seal = true on the same stream, which records ONE event for all
// of them.  The pool touches a stream only inside such calls of the stream's user, or -- for unsealed batches -- later: the caller
// leaves a batch unsealed only while it vouches for the stream's life (a plan on a caller's stream seals at fg_plan_destroy at the
// latest; the library's own cached streams are never destroyed; whoever destroys a stream that plans ran on calls retire(stream)
// first).  Recording every batch at its put cost 9 us per plan on the
// MI355X (profiles/stream_ordered_plans_summary.md).  An event goes back to the event cache when the last block that shares it
// leaves the free list.
// The bookkeeping knows nothing of HIP: every device call goes through the policy H, so that tests/hostcheck/pool_check.cpp
// compiles this header on the host against a policy that counts the calls.  H provides
//   typedef Stream, Event;
//   static void *dev_malloc(size_t);  static void dev_free(void *);
//   static Event event_get(int dev);  static void event_put(int dev, Event);      (a cache of ordering-only events)
//   static void event_record(int dev, Event, Stream);  static bool event_passed(Event);
//   static void stream_wait(Stream, Event);   static void event_wait_host(Event);
//   static bool poison_on();  static void poison(void *, size_t);                 (FREGRID_HIP_POISON)
#pragma once
#include <stddef.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

template <class H> struct DevPool {
  typedef typename H::Stream Stream;
  typedef typename H::Event Event;
  struct Ev { Event ev; int dev; int refs; };                               // one recorded event, shared by batches
  struct Batch { Ev *e; Stream stream; int dev; int refs; };                // e null: no event yet
  struct FreeBlock { void *p; Batch *batch; };                              // batch null: untagged
  std::mutex mu;
  std::map<std::pair<int, size_t>, std::vector<FreeBlock>> free_;          // (device, class bytes) -> blocks
  std::map<void *, std::pair<int, size_t>> live_;
  std::vector<Batch *> open_;                                              // batches without an event
  long events_ = 0;                                                        // events held

  static size_t klass(size_t n)
  {
    size_t c = 256;
    while (c < n) c += (c < (1u << 20) ? c : (c >> 2));                     // x2 up to 1 MiB, then x1.25
    return c;
  }
  size_t block_bytes(void *p) { std::lock_guard<std::mutex> lk(mu); auto it = live_.find(p); return it == live_.end() ? 0 : it->second.second; }   // class bytes of a block in use
  long live_events() { std::lock_guard<std::mutex> lk(mu); return events_; }
  size_t cached_blocks() { std::lock_guard<std::mutex> lk(mu); size_t n = 0; for (auto &kv : free_) n += kv.second.size(); return n; }

  void *get(int dev, size_t n) { return hand_out(take(dev, n, false, Stream()), n); }
  void *get(int dev, size_t n, Stream stream) { return hand_out(take(dev, n, true, stream), n); }

  void put(void *p) { put_many(&p, 1, false, Stream(), false); }
  void put(void *p, Stream stream, bool seal_now) { put_many(&p, 1, true, stream, seal_now); }
  void put(const std::vector<void *> &ps, Stream stream, bool seal_now) { put_many(ps.data(), ps.size(), true, stream, seal_now); }   // one batch

  // one event, recorded now, for every batch of `stream` that has none: afterwards the pool does not touch the stream again
  void seal(Stream stream) { std::lock_guard<std::mutex> lk(mu); seal_locked(stream); }

  // The caller has synchronised `stream` and is about to destroy it.  Nothing on the device uses the stream's blocks any more, so
  // they become untagged and their events go back to the cache: no event that was recorded on the stream stays in the pool.  (The
  // runtime follows an event back to the stream it was recorded on when it is asked about the event -- hipEventQuery on an event of
  // a destroyed stream reads freed memory and has answered "operation not permitted when stream is capturing".)
  void retire(Stream stream)
  {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &kv : free_)
      for (FreeBlock &b : kv.second)
        if (b.batch && b.batch->stream == stream) { Batch *t = b.batch; b.batch = nullptr; unref(t); }
  }

  // waits for every tagged block's batch, then frees every cached block
  void release_all()
  {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &kv : free_) for (FreeBlock &b : kv.second) if (b.batch) { H::event_wait_host(event_of(b.batch)); unref(b.batch); b.batch = nullptr; }
    for (auto &kv : free_) for (FreeBlock &b : kv.second) H::dev_free(b.p);
    free_.clear();
  }

 private:
  void seal_locked(Stream stream)
  {
    Ev *e = nullptr;
    for (size_t k = 0; k < open_.size();) {
      Batch *b = open_[k];
      if (!(b->stream == stream)) { k++; continue; }
      if (!e) { e = new Ev{H::event_get(b->dev), b->dev, 0}; events_++; H::event_record(b->dev, e->ev, stream); }
      b->e = e; e->refs++;
      open_.erase(open_.begin() + k);
    }
  }
  Event event_of(Batch *b)
  {
    if (!b->e) seal_locked(b->stream);
    return b->e->ev;
  }
  void unref(Batch *b)
  {
    if (--b->refs > 0) return;
    if (b->e) { if (--b->e->refs == 0) { H::event_put(b->e->dev, b->e->ev); events_--; delete b->e; } }
    else open_.erase(std::find(open_.begin(), open_.end(), b));
    delete b;
  }
  // FREGRID_HIP_POISON=1 (tests): every block handed out is filled with 0x7f bytes first, so that a kernel reading something it
  // or its predecessors never wrote meets wild indices / NaN-like doubles instead of a lucky zero or a stale valid value.  The
  // fill synchronises the whole device before and after itself, whatever the block's tag said.
  void *hand_out(void *p, size_t n)
  {
    if (p && H::poison_on()) H::poison(p, klass(n ? n : 1));
    return p;
  }
  void *take(int dev, size_t n, bool on_stream, Stream stream)
  {
    if (n == 0) n = 1;
    const size_t c = klass(n);
    {
      std::lock_guard<std::mutex> lk(mu);
      auto it = free_.find({dev, c});
      if (it != free_.end() && !it->second.empty()) {
        std::vector<FreeBlock> &v = it->second;
        // the newest block that can go out as it is (0: untagged, or tagged with the asking stream -- newest first, as the pool
        // always did: the block given back last is the one still in the caches); else one whose batch's event has passed (2);
        // else the oldest of those that need a wait (3)
        int best = -1, best_rank = 4;
        for (int k = (int)v.size() - 1; k >= 0 && best_rank > 0; k--) {
          const Batch *b = v[k].batch;
          const int rank = (!b || (on_stream && b->stream == stream)) ? 0 : 3;
          if (rank < best_rank || (rank == 3 && best_rank == 3)) { best = k; best_rank = rank; }
        }
        if (best_rank == 3)
          for (int k = (int)v.size() - 1; k >= 0; k--)
            if (v[k].batch->e && H::event_passed(v[k].batch->e->ev)) { best = k; best_rank = 2; break; }
        FreeBlock fb = v[best];
        v.erase(v.begin() + best);
        if (fb.batch) {
          if (best_rank == 3) { if (on_stream) H::stream_wait(stream, event_of(fb.batch)); else H::event_wait_host(event_of(fb.batch)); }
          unref(fb.batch);
        }
        live_[fb.p] = {dev, c};
        return fb.p;
      }
    }
    void *p = H::dev_malloc(c);
    if (!p) {
      release_all();
      p = H::dev_malloc(c);
      if (!p) return nullptr;
    }
    std::lock_guard<std::mutex> lk(mu);
    live_[p] = {dev, c};
    return p;
  }
  // a null pointer, a pointer the pool does not know and a block that is already back are ignored
  void put_many(void *const *ps, size_t n, bool tagged, Stream stream, bool seal_now)
  {
    std::lock_guard<std::mutex> lk(mu);
    Batch *b = nullptr;
    for (size_t k = 0; k < n; k++) {
      auto it = live_.find(ps[k]);
      if (!ps[k] || it == live_.end()) continue;
      if (tagged && !b) { b = new Batch{nullptr, stream, it->second.first, 0}; open_.push_back(b); }
      if (b) b->refs++;
      free_[it->second].push_back(FreeBlock{ps[k], b});
      live_.erase(it);
    }
    if (tagged && seal_now) seal_locked(stream);
  }
};
