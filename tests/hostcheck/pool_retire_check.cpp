// pool_retire_check.cpp -- DevPool::retire (csrc/dev_pool.h) on the host, against a policy that keeps count of the events the pool
// holds and of the stream each was recorded on.  usage: pool_retire_check; prints "ok" and exits 0, or says what failed and exits 1.
// tests/test_dev_pool_retire_cpu.py builds it with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <vector>
#include "dev_pool.h"

struct FakeEvent { bool passed = false; int stream = -1; };
struct Fake {
  typedef int Stream;
  typedef FakeEvent *Event;
  static int stream_waits, host_waits, queries_on_dead;
  static std::set<Event> out;            // events the pool holds
  static std::set<int> dead;             // destroyed streams
  static void *dev_malloc(size_t) { return malloc(16); }
  static void dev_free(void *p) { free(p); }
  static Event event_get(int) { Event e = new FakeEvent; out.insert(e); return e; }
  static void event_put(int, Event e) { out.erase(e); delete e; }
  static void event_record(int, Event e, Stream s) { if (dead.count(s)) queries_on_dead++; e->stream = s; e->passed = false; }
  static bool event_passed(Event e) { if (dead.count(e->stream)) queries_on_dead++; return e->passed; }
  static void stream_wait(Stream, Event e) { if (dead.count(e->stream)) queries_on_dead++; stream_waits++; }
  static void event_wait_host(Event e) { if (dead.count(e->stream)) queries_on_dead++; host_waits++; e->passed = true; }
  static bool poison_on() { return false; }
  static void poison(void *, size_t) {}
};
int Fake::stream_waits, Fake::host_waits, Fake::queries_on_dead;
std::set<Fake::Event> Fake::out;
std::set<int> Fake::dead;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main()
{
  DevPool<Fake> pool;
  // stream 1: a sealed batch of two blocks and an open (unsealed) batch of one; stream 2: a sealed batch of one
  void *a = pool.get(0, 1000, 1), *b = pool.get(0, 1000, 1), *c = pool.get(0, 5000, 1), *d = pool.get(0, 1000, 2);
  pool.put(std::vector<void *>{a, b}, 1, true);
  pool.put(c, 1, false);
  pool.put(d, 2, true);
  CHECK(pool.live_events() == 2 && Fake::out.size() == 2 && pool.cached_blocks() == 4);
  // the user of stream 1 has synchronised it and destroys it
  pool.retire(1);
  Fake::dead.insert(1);
  CHECK(pool.live_events() == 1 && Fake::out.size() == 1);            // stream 2's event stays
  CHECK((*Fake::out.begin())->stream == 2);
  CHECK(pool.cached_blocks() == 4);                                  // the blocks stay cached
  // the retired blocks go out as untagged ones: to another stream without a wait, to a streamless caller without a host wait, and
  // the open batch never gets its event recorded on the dead stream
  void *x = pool.get(0, 5000, 3);
  CHECK(x == c && Fake::stream_waits == 0);
  void *y = pool.get(0, 1000), *z = pool.get(0, 1000);
  CHECK((y == a || y == b) && (z == a || z == b) && y != z && Fake::host_waits == 0);
  CHECK(Fake::queries_on_dead == 0);
  // stream 2's block still needs its event
  void *w = pool.get(0, 1000, 3);
  CHECK(w == d && Fake::stream_waits == 1 && pool.live_events() == 0);
  // retiring a stream the pool knows nothing of, and twice, changes nothing
  pool.retire(7); pool.retire(1);
  CHECK(pool.cached_blocks() == 0 && pool.live_events() == 0);
  for (void *p : {x, y, z, w}) pool.put(p);
  pool.release_all();
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
