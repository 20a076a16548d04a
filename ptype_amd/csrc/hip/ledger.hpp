// Send ledger (ledger.hip, ops/ledger.py): what a rank's Sends carried, kept in
// HBM and read only by Stats().  One block of int64 words; every Send's final
// replies are folded into it by one kernel (launch_ledger_account), no host read.
//
// The block is kept in kLedgerCopies copies, kLedgerWords apart: block b of a
// launch adds to copy b % kLedgerCopies, and a reader folds the copies (sum; xor
// for digest_xor).  Atomics of many blocks to one word -- or to words of one cache
// line -- serialise at the memory side, 7-10 ns each: the 8 Mi-message pass took
// 64.5 us with a single copy and takes 38.6 us with 16 (profiles/ledger.md).
//
// Word layout (ops/ledger.py mirrors it; `ledger_words()` exports it to the tests):
//   [0, 128)  calls[method slot][status slot]: messages per (method, status)
//             method slot: the method id read as u16, ids 0..14 their own slot, every
//             other id (kMethodRelay, kMethodCoordPrime, garbage) slot 15 "other"
//             status slot: 0..6 their own slot, anything else (negative, >= 7) slot 7
//   messages  messages accounted
//   sends     launches (one per Send, also for an empty one); both are added once per
//             launch, by the block that wins last_block_ticket (common.hpp)
//   digest_sum / digest_xor   wrapping sum and xor over all messages of
//               h(i, v, s) = mix64(mix64(i + 1) ^ (uint64)v' ^ ((uint64)(uint32)s * kLedgerGold))
//             i: the message's index in its Send; v' = value when s == kStatusOk, else 0
//             (a failed reply's value is no part of any contract); mix64: common.hpp
//   audited / mismatch   OK replies of kCalculatorMultiply (a0 * a1, wrapping) and kEcho
//             (a0) recomputed from the batch: how many were compared, how many differ
//   load_oob  messages whose actor id (as u32) is past the per-actor load table
#pragma once
#include <stdint.h>

namespace ptype {

constexpr int kLedgerMethodSlots = 16;
constexpr int kLedgerStatusSlots = 8;
constexpr int kLedgerCalls = 0;
constexpr int kLedgerMessages = kLedgerMethodSlots * kLedgerStatusSlots;  // 128
constexpr int kLedgerSends = kLedgerMessages + 1;
constexpr int kLedgerDigestSum = kLedgerMessages + 2;
constexpr int kLedgerDigestXor = kLedgerMessages + 3;
constexpr int kLedgerAudited = kLedgerMessages + 4;
constexpr int kLedgerMismatch = kLedgerMessages + 5;
constexpr int kLedgerLoadOob = kLedgerMessages + 6;
constexpr int kLedgerWords = kLedgerMessages + 8;  // (one spare word: 16-byte multiple)
constexpr int kLedgerCopies = 16;

constexpr uint64_t kLedgerGold = 0x9e3779b97f4a7c15ull;

}  // namespace ptype
