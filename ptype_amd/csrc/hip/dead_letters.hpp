// Dead-letter queue (dead_letters.hip, ops/dead_letters.py): the calls of a rank's Sends
// that still failed after every wrapper, kept in HBM with the whole call, so that they
// can be looked at and re-sent (redrive) after the caller's batch is gone.
//
// A ring of `entries` records (a power of two in [64, 2^24]) and one 64-byte control
// line.  Letter t -- tickets count the letters ever appended -- lives in slot
// t & (entries - 1).  Word layout (ops/dead_letters.py mirrors it; `dead_letter_layout()`
// exports it to the tests):
//
//   record, 8 u64 words (64 B)
//     w0  ticket + 1 (0: never written)
//     w1  `sends` after the Send that filed it (the first Send is 1)
//     w2  row u32 | status i32 << 32
//     w3  logical actor id u32 | method u16 << 32 | attempts u16 << 48
//     w4  a0      w5  a1 (0 without the column)      w6  a2 (alike)      w7  tag
//
//   control line, 8 u64 words
//     head     letters ever appended
//     tail     the first unread ticket
//     dropped  letters overwritten (or, of more than `entries` in one Send, never
//              written) before anyone took them
//     sends    dead-lettered Sends, also those without a letter
//     base     kernel scratch: `head` as the Send's count launch found it -- the append
//              launch reads this word and never `head`, which its last block commits
//     torn     slots whose ticket word was not the expected one when taken (stays 0)
//     seq      kernel scratch: `sends` + 1 of the Send being filed, alike
#pragma once
#include <stdint.h>

namespace ptype {

constexpr int kDlqRecordWords = 8;
constexpr int kDlqTicket = 0, kDlqSeq = 1, kDlqRowStatus = 2, kDlqActorMethodAttempts = 3;
constexpr int kDlqA0 = 4, kDlqA1 = 5, kDlqA2 = 6, kDlqTag = 7;

constexpr int kDlqCtrlWords = 8;
constexpr int kDlqHead = 0, kDlqTail = 1, kDlqDropped = 2, kDlqSends = 3, kDlqBase = 4, kDlqTorn = 5, kDlqSeqNext = 6;

constexpr int64_t kDlqMinEntries = 64, kDlqMaxEntries = 1 << 24;
constexpr unsigned kDlqMaxAttempts = 65535;

}  // namespace ptype
