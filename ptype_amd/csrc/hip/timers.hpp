// Timer queue (timers.hip, ops/timers.py): delayed messages kept in HBM.  Schedule files a
// batch with a per-row delay in ticks, Tick advances the runtime's clock by one and takes
// the messages that are due.  There is no wall clock: every word below is a function of
// the calls alone.
//
// Word layout (ops/timers.py mirrors it; `timer_layout()` exports it to the tests):
//
//   ring: `entries` records (a power of two in [64, 2^24]); record t -- tickets count the
//   records ever filed -- lives in slot t & (entries - 1).  A record is 8 u64 words (64 B):
//     w0  ticket + 1 (0: never written)
//     w1  due tick (the clock at Schedule + delay)
//     w2  row u32 | delay u32 << 32
//     w3  logical actor id u32 | method u16 << 32
//     w4  a0      w5  a1 (0 without the column)      w6  a2 (alike)      w7  tag
//
//   run table: `runs` descriptors (a power of two in [4, 4096]); run q -- the accepted rows
//   of one Schedule, stored sorted by (delay, row) in consecutive tickets -- lives in slot
//   q & (runs - 1).  A descriptor is a 64-B header
//     t0         the clock when the run was scheduled
//     base       the run's first ticket
//     n          its records
//     max_delay  its largest delay: the run is finished once now >= t0 + max_delay
//     seq        q + 1
//   followed by off[horizon + 2] u32, padded to 64 B: off[d] is the number of the run's
//   records with a delay < d, so the records due at t0 + d are the tickets
//   [base + off[d], base + off[d + 1]).  `horizon` is a power of two in [16, 1024].
//
//   control line, 8 u64 words
//     now        the clock, in ticks
//     head       records ever filed
//     tail       the base of the oldest run that is not finished (head without one): the
//                ring holds [tail, head)
//     runs_head  runs ever filed
//     runs_tail  the oldest run that is not finished
//     refused    rows whose delay was outside [1, horizon], never filed
//     delivered  records ever due
//     torn       records whose ticket word was not the expected one when taken (stays 0)
//
//   scratch line, 8 u64 words: what the kernels hand to the host and to each other; no
//   part of the queue's state
//     k, max_delay                 of the Schedule being filed (timer_scan_kernel)
//     refused                      the control line's `refused` as it is after that Schedule
//     head, runs_head, now         the control words as that Schedule found them -- the file
//                                  launch reads these and never the control words, which
//                                  its last block commits
//     n_due, segs                  of the last Tick (timer_due_kernel): the records due and
//                                  the live runs whose segments the take launch searches
#pragma once
#include <stdint.h>

namespace ptype {

constexpr int kTmrRecordWords = 8;
constexpr int kTmrTicket = 0, kTmrDue = 1, kTmrRowDelay = 2, kTmrActorMethod = 3;
constexpr int kTmrA0 = 4, kTmrA1 = 5, kTmrA2 = 6, kTmrTag = 7;

constexpr int kTmrHeaderWords = 8;  // u64 words of a run descriptor's header
constexpr int kTmrT0 = 0, kTmrBase = 1, kTmrN = 2, kTmrMaxDelay = 3, kTmrSeq = 4;

constexpr int kTmrCtrlWords = 8;
constexpr int kTmrNow = 0, kTmrHead = 1, kTmrTail = 2, kTmrRunsHead = 3, kTmrRunsTail = 4, kTmrRefused = 5,
              kTmrDelivered = 6, kTmrTorn = 7;

constexpr int kTmrScratchWords = 8;
constexpr int kTmrSK = 0, kTmrSRefused = 1, kTmrSMaxDelay = 2, kTmrSHead = 3, kTmrSRunsHead = 4, kTmrSNow = 5,
              kTmrSDue = 6, kTmrSSegs = 7;

constexpr int64_t kTmrMinEntries = 64, kTmrMaxEntries = 1 << 24;
constexpr int64_t kTmrMinHorizon = 16, kTmrMaxHorizon = 1024;
constexpr int64_t kTmrMinRuns = 4, kTmrMaxRuns = 4096;

// u64 words of one run descriptor: the header and off[horizon + 2] u32 padded to 64 B
constexpr int64_t timer_desc_words(int64_t horizon) { return kTmrHeaderWords + ((horizon + 2 + 15) / 16) * 8; }

}  // namespace ptype
