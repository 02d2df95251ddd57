// tests/c/ahead_model.h -- the device model of the look-ahead sweeps (ahead_sweep.cpp: csrc/xl_ahead.h; q15_ahead_sweep.cpp:
// csrc/xl_q15_ahead.h), each a stand-alone host program that includes this once:
//   - a stream is a vector clock; a launch ticks its stream and carries the clock; X happens before Y iff Y's clock has reached X's tick
//     of X's stream
//   - an event holds the clock of its latest record; a wait joins it into the waiting stream (HIP: the latest record enqueued before the
//     wait -- the host enqueues in program order, so that is the event's current value); a never-recorded event is no wait
//   - every phase table and phase buffer remembers its writer, the latest tick per stream of its readers, and WHAT it holds: a table the
//     phases it started from and the position and shape it was tabulated for, a buffer a hash chained over every call's shape
// res_read and res_write carry the two orderings every sweep checks: a reader comes after the writer of what it reads, a writer after
// the earlier writer and every earlier reader.
#ifndef AHEAD_MODEL_H_
#define AHEAD_MODEL_H_

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { ST_A, ST_B, ST_OWN, ST_CS_MASKED, ST_NCO, ST_NCO_MASKED, NST };  // two caller streams, the engine's streams

static unsigned long g_checks = 0;
static char g_ctx[512];
#define CHECK(cond)                                                                 \
  do {                                                                              \
    ++g_checks;                                                                     \
    if (!(cond)) {                                                                  \
      fprintf(stderr, "FAIL %s:%d: %s | %s\n", __FILE__, __LINE__, #cond, g_ctx); \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

struct Clock {
  uint32_t t[NST];
};
struct Event {
  bool recorded;
  Clock c;
};
struct Op {
  int s;
  Clock c;
};
struct Res {  // a phase table or a phase buffer
  int wstream;  // -1: initialised by the host
  uint32_t wtick;
  uint32_t rtick[NST];
  uint64_t hash;  // buffer: the phases it holds; table: the phases it was tabulated from
  uint32_t trel, S, G, flags;
};
struct Shape {
  uint32_t S, G, flags;
};
struct Streams {  // a sweep's model of the engine derives from this
  Clock st[NST];
};

static inline uint64_t mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  return h * 0xD6E8FEB86659FD93ull;
}
static inline uint64_t step_hash(uint64_t h, Shape sh) { return mix(mix(mix(h, sh.S), sh.G), sh.flags + 11u); }

static inline Op launch(Streams &m, int s) {
  m.st[s].t[s]++;
  const Op o = {s, m.st[s]};
  return o;
}
static inline void record(Streams &m, Event &e, int s) { e.recorded = true, e.c = m.st[s]; }
static inline void wait(Streams &m, int s, const Event &e) {
  if (!e.recorded) return;
  for (int i = 0; i < NST; ++i)
    if (e.c.t[i] > m.st[s].t[i]) m.st[s].t[i] = e.c.t[i];
}
static inline void sync_all(Streams &m) {  // xl_batch_sync_all: the host waits for every stream
  Clock j = m.st[0];
  for (int s = 1; s < NST; ++s)
    for (int i = 0; i < NST; ++i)
      if (m.st[s].t[i] > j.t[i]) j.t[i] = m.st[s].t[i];
  for (int s = 0; s < NST; ++s) m.st[s] = j;
}
static inline bool written_before(const Res &r, const Op &o) { return r.wstream < 0 || r.wtick <= o.c.t[r.wstream]; }
static inline void res_read(Res &r, const Op &o) {
  CHECK(written_before(r, o));  // (a): the reader comes after the tabulation that wrote what it reads
  if (o.c.t[o.s] > r.rtick[o.s]) r.rtick[o.s] = o.c.t[o.s];
}
static inline void res_write(Res &r, const Op &o) {
  CHECK(written_before(r, o));
  for (int s = 0; s < NST; ++s) CHECK(r.rtick[s] <= o.c.t[s]);  // (b): every earlier reader has happened
  r.wstream = o.s, r.wtick = o.c.t[o.s];
  memset(r.rtick, 0, sizeof(r.rtick));
}

#endif  // AHEAD_MODEL_H_
