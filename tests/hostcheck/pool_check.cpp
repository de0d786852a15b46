// pool_check.cpp -- csrc/dev_pool.h compiled for the host against a policy that counts the device calls and whose events pass
// when the test says so.  usage: pool_check CASE; prints "ok CASE" and exits 0, or says what failed and exits 1.
// tests/test_dev_pool_cpu.py builds it with -fsanitize=address,undefined and runs every case.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>
#include <vector>
#include "dev_pool.h"

struct FakeEvent { bool passed = false; int records = 0; int id = 0; int stream = -1; };
struct Fake {
  typedef int Stream;                 // streams are small numbers
  typedef FakeEvent *Event;
  static int mallocs, frees, stream_waits, host_waits, host_waits_unpassed, created, poisons;
  static std::vector<Event> cache;
  static std::set<Event> out;        // events the pool holds
  static std::vector<std::pair<Stream, Event>> waits;
  static std::vector<std::string> log;    // "wait" / "free" in call order (release_all)
  static bool fail_malloc;
  static void *dev_malloc(size_t c) { if (fail_malloc) return nullptr; mallocs++; return malloc(c < 64 ? c : 64); }
  static void dev_free(void *p) { frees++; log.push_back("free"); free(p); }
  static Event event_get(int)
  {
    Event e;
    if (!cache.empty()) { e = cache.back(); cache.pop_back(); } else { e = new FakeEvent; e->id = created++; }
    e->passed = false; e->records = 0;
    out.insert(e);
    return e;
  }
  static void event_put(int, Event e) { out.erase(e); cache.push_back(e); }
  static void event_record(int, Event e, Stream s) { e->records++; e->stream = s; e->passed = false; }
  static bool event_passed(Event e) { return e->passed; }
  static void stream_wait(Stream s, Event e) { stream_waits++; waits.push_back({s, e}); }
  static void event_wait_host(Event e) { host_waits++; if (!e->passed) host_waits_unpassed++; e->passed = true; log.push_back("wait"); }
  static bool poison_on() { return false; }
  static void poison(void *, size_t) { poisons++; }
  static void reset()
  {
    mallocs = frees = stream_waits = host_waits = host_waits_unpassed = poisons = 0;
    waits.clear(); log.clear(); fail_malloc = false;
  }
  static void drop_cache() { for (Event e : cache) delete e; cache.clear(); }
};
int Fake::mallocs, Fake::frees, Fake::stream_waits, Fake::host_waits, Fake::host_waits_unpassed, Fake::created, Fake::poisons;
std::vector<Fake::Event> Fake::cache;
std::set<Fake::Event> Fake::out;
std::vector<std::pair<int, Fake::Event>> Fake::waits;
std::vector<std::string> Fake::log;
bool Fake::fail_malloc;

typedef DevPool<Fake> P;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static Fake::Event only_event() { return Fake::out.size() == 1 ? *Fake::out.begin() : nullptr; }

static void same_stream()
{
  P pool;
  void *a = pool.get(0, 1000, 1);
  CHECK(Fake::mallocs == 1);
  pool.put(a, 1, false);
  CHECK(pool.cached_blocks() == 1 && pool.live_events() == 0);
  void *b = pool.get(0, 900, 1);                     // same class (1024), same stream: as it is
  CHECK(b == a && Fake::mallocs == 1 && Fake::stream_waits == 0 && Fake::host_waits == 0);
  CHECK(Fake::created == 0 && Fake::out.empty());    // a batch that goes back to its own stream never costs an event
  pool.put(b);
  pool.release_all();
  CHECK(Fake::frees == 1 && Fake::host_waits == 0);
}
static void cross_stream()
{
  P pool;
  void *a = pool.get(0, 5000, 1), *b = pool.get(0, 5000, 1);
  pool.put(std::vector<void *>{a, b}, 1, false);            // one batch
  CHECK(pool.live_events() == 0);                    // its event is recorded when somebody needs it
  void *c = pool.get(0, 5000, 2);
  Fake::Event ev = only_event();
  CHECK(ev && ev->records == 1 && ev->stream == 1 && pool.live_events() == 1);      // recorded once, on the batch's stream
  CHECK((c == a || c == b) && Fake::mallocs == 2 && Fake::host_waits == 0);
  CHECK(Fake::stream_waits == 1 && Fake::waits.size() == 1 && Fake::waits[0].first == 2 && Fake::waits[0].second == ev);
  ev->passed = true;
  void *d = pool.get(0, 5000, 3);                    // the batch's other block: the event has passed, and is not recorded again
  CHECK((d == a || d == b) && d != c && Fake::stream_waits == 1 && Fake::host_waits == 0 && Fake::mallocs == 2 && ev->records == 1);
  CHECK(pool.live_events() == 0 && Fake::out.empty() && Fake::cache.size() == 1);
  // not passed: each taker queues its own wait on the one event
  pool.put(std::vector<void *>{c, d}, 2, false);
  void *e = pool.get(0, 5000, 1), *f = pool.get(0, 5000, 3);
  CHECK(Fake::stream_waits == 3 && Fake::waits[1].first == 1 && Fake::waits[2].first == 3 && Fake::waits[1].second == Fake::waits[2].second);
  CHECK(Fake::waits[1].second->records == 1 && Fake::waits[1].second->stream == 2 && pool.live_events() == 0);
  pool.put(e); pool.put(f);
  pool.release_all();
  CHECK(Fake::frees == 2 && Fake::host_waits == 0);
}
static void streamless()
{
  P pool;
  void *t = pool.get(0, 300, 1), *u = pool.get(0, 300, 1), *w = pool.get(0, 300, 1);
  pool.put(u);                                       // untagged
  pool.put(std::vector<void *>{t, w}, 1, false);            // tagged, newer
  void *x = pool.get(0, 300);
  CHECK(x == u && Fake::host_waits == 0 && Fake::stream_waits == 0 && Fake::created == 0);      // prefers the untagged block
  void *y = pool.get(0, 300);                        // only tagged blocks are left, nothing has passed: a host wait, no malloc
  CHECK(y == t && Fake::host_waits == 1 && Fake::host_waits_unpassed == 1 && Fake::mallocs == 3 && Fake::stream_waits == 0);
  CHECK(pool.live_events() == 1 && only_event()->records == 1 && only_event()->stream == 1);
  void *z = pool.get(0, 300);                        // the batch's event has passed (the wait above): no second wait
  CHECK(z == w && Fake::host_waits == 1 && pool.live_events() == 0);
  void *n = pool.get(0, 300);                        // an empty class allocates
  CHECK(n && Fake::mallocs == 4);
  // of the pending blocks one whose event has passed is taken without a wait
  pool.put(std::vector<void *>{x, z}, 4, false);
  pool.put(std::vector<void *>{y, n}, 5, false);
  void *q = pool.get(0, 300, 9);                     // oldest first: x, behind a queued wait on batch 4's event
  Fake::Event e4 = only_event();
  CHECK(q == x && e4 && e4->stream == 4 && Fake::stream_waits == 1);
  e4->passed = true;
  void *r = pool.get(0, 300);
  CHECK(r == z && Fake::host_waits == 1 && Fake::mallocs == 4);
  void *v = pool.get(0, 300);                        // batch 5: never recorded so far, so not passed
  CHECK(v == y && Fake::host_waits == 2 && Fake::host_waits_unpassed == 2 && Fake::mallocs == 4);
  pool.put(q); pool.put(r); pool.put(v);
  pool.release_all();                                // (n is still in batch 5, whose event the wait above has seen pass)
  CHECK(Fake::frees == 4);
}
static void seal()
{
  P pool;
  void *a = pool.get(0, 100, 1), *b = pool.get(0, 100, 1), *c = pool.get(0, 100, 2), *d = pool.get(0, 100, 1);
  pool.put(std::vector<void *>{a}, 1, false);        // two unsealed batches of stream 1, one of stream 2
  pool.put(std::vector<void *>{c}, 2, false);
  pool.put(std::vector<void *>{b}, 1, false);
  CHECK(pool.live_events() == 0 && Fake::created == 0);
  pool.put(std::vector<void *>{d}, 1, true);         // the sealing put: ONE event, recorded now, for all three batches of stream 1
  Fake::Event e1 = only_event();
  CHECK(e1 && e1->records == 1 && e1->stream == 1 && pool.live_events() == 1);
  void *x = pool.get(0, 100, 3);                     // oldest first: a, on the sealed event, no new record
  CHECK(x == a && Fake::stream_waits == 1 && Fake::waits[0].second == e1 && e1->records == 1);
  void *y = pool.get(0, 100, 3);                     // then c, of stream 2: its own event, recorded now
  CHECK(y == c && Fake::stream_waits == 2 && Fake::waits[1].second != e1 && Fake::waits[1].second->stream == 2);
  pool.seal(2);                                      // nothing of stream 2 is left without an event: no record
  pool.seal(1);
  CHECK(Fake::created == 2 && e1->records == 1);
  e1->passed = true;
  void *z = pool.get(0, 100), *w = pool.get(0, 100);            // b and d share the event with a: passed for all
  CHECK(z && w && Fake::host_waits == 0 && Fake::mallocs == 4 && pool.live_events() == 0 && Fake::out.empty());
  pool.put(x); pool.put(y); pool.put(z); pool.put(w);
  pool.release_all();
  CHECK(Fake::frees == 4 && Fake::host_waits == 0);
}
static void release_all_waits()
{
  P pool;
  void *a = pool.get(0, 100, 1), *b = pool.get(0, 70000, 2), *c = pool.get(1, 100, 1);
  pool.put(a, 1, false); pool.put(b, 2, false); pool.put(c);
  CHECK(pool.live_events() == 0 && pool.cached_blocks() == 3);
  pool.release_all();
  CHECK(Fake::host_waits == 2 && Fake::frees == 3 && pool.live_events() == 0 && pool.cached_blocks() == 0 && Fake::out.empty());
  bool seen_free = false, ordered = true;
  for (const std::string &s : Fake::log) { if (s == "free") seen_free = true; else if (seen_free) ordered = false; }
  CHECK(ordered);                                    // every wait comes before the first free
  // an allocation failure releases the cache (waiting first) and tries again
  void *d = pool.get(0, 100, 1);
  pool.put(d, 1, false);
  Fake::fail_malloc = true;
  CHECK(pool.get(0, 1 << 20, 1) == nullptr && pool.cached_blocks() == 0 && Fake::host_waits == 3);
}
static void events_bounded()
{
  P pool;
  size_t most_out = 0;
  std::vector<void *> held;
  for (int round = 0; round < 1000; round++) {
    std::vector<void *> blocks;
    for (int k = 0; k < 5; k++) blocks.push_back(pool.get(0, 256 << k, round % 3));
    if (round % 7 == 0) { void *p = blocks.back(); blocks.pop_back(); pool.put(p, (round + 1) % 3, false); }   // a batch of its own
    pool.put(blocks, round % 3, round % 2 == 0);
    if (round % 5 == 0) for (FakeEvent *e : Fake::out) e->passed = true;
    if (Fake::out.size() > most_out) most_out = Fake::out.size();
    CHECK((long)Fake::out.size() == pool.live_events());
  }
  CHECK(most_out <= 10);                             // five classes, one block each: at most a batch per cached block
  CHECK(Fake::created <= 12);                        // the cache is reused: no event per round
  CHECK(Fake::mallocs <= 10);
  CHECK(Fake::host_waits == 0);
  pool.release_all();
  CHECK(Fake::out.empty() && pool.live_events() == 0);
}
static void classes()
{
  const size_t in[] = {0, 1, 255, 256, 257, 1000, 4096, 4097, 1u << 20, (1u << 20) + 1, 1310720, 1310721, 3000000, 100000000};
  const size_t want[] = {256, 256, 256, 256, 512, 1024, 4096, 8192, 1048576, 1310720, 1310720, 1638400, 3200000, 113686827};
  for (size_t k = 0; k < sizeof(in) / sizeof(in[0]); k++) {
    if (P::klass(in[k]) != want[k]) printf("klass(%zu) = %zu, want %zu\n", in[k], P::klass(in[k]), want[k]);
    CHECK(P::klass(in[k]) == want[k]);
  }
  P pool;
  void *a = pool.get(0, 0);                          // a request of nothing is a block of the smallest class
  pool.put(a);
  CHECK(pool.get(0, 200) == a);
  pool.put(a);
  void *b = pool.get(1, 200);                        // another device: another list
  CHECK(b != a && Fake::mallocs == 2);
  pool.put(b);
  pool.release_all();
}
static void ignored_puts()
{
  P pool;
  void *a = pool.get(0, 100, 1);
  int local = 0;
  pool.put(nullptr); pool.put(nullptr, 1, false); pool.put(&local); pool.put(&local, 1, false);
  CHECK(pool.cached_blocks() == 0 && pool.live_events() == 0 && Fake::out.empty());      // no event for a batch of nothing
  pool.put(a, 1, false);
  pool.put(a, 1, false); pool.put(a);                       // already back
  CHECK(pool.cached_blocks() == 1);
  pool.put(std::vector<void *>{nullptr, &local, a}, 2, false);
  CHECK(pool.cached_blocks() == 1);
  void *b = pool.get(0, 100, 1), *c = pool.get(0, 100, 1);
  CHECK(b == a && c != a && Fake::mallocs == 2 && Fake::created == 0 && Fake::stream_waits == 0);      // still tagged with stream 1, once
  pool.put(b); pool.put(c);
  pool.release_all();
  CHECK(Fake::frees == 2);
}

int main(int argc, char **argv)
{
  struct { const char *name; void (*fn)(); } cases[] = {
    {"same_stream", same_stream}, {"cross_stream", cross_stream}, {"streamless", streamless}, {"release_all", release_all_waits}, {"seal", seal},
    {"events_bounded", events_bounded}, {"classes", classes}, {"ignored_puts", ignored_puts}};
  if (argc != 2) { printf("usage: pool_check CASE\n"); return 2; }
  for (auto &c : cases)
    if (!strcmp(argv[1], c.name)) {
      Fake::reset();
      c.fn();
      if (!Fake::out.empty()) { printf("FAILED: %zu events still out at the end\n", Fake::out.size()); fails++; }
      Fake::drop_cache();
      if (!fails) printf("ok %s\n", c.name);
      return fails ? 1 : 0;
    }
  printf("no such case: %s\n", argv[1]);
  return 2;
}
