// Reply gather (gather.hip, ops/gather.py): the M replies of one Send folded into G
// groups on the device -- the gather half of a scatter-gather (the reference's
// watchReplies, example/optimus/coordinator.go:91-98, for any grouping and op).
//
// Ops over the STATUS_OK rows of a group (rows in message order):
//   sum       wrapping mod 2^64, 0 without an OK row
//   min, max  signed; INT64_MAX / INT64_MIN without an OK row
//   first_ne  the value of the lowest OK row that differs from the group's sentinel,
//             unless a non-OK row lies below it (or there is none): then the sentinel
//
// Accumulator: kGatherAccWords u64 per group, then one more row whose first word
// counts the rows with a group id >= G (`oob`):
//   word 0  the folded value (the op's identity between reduces; unused by first_ne)
//   word 1  count << 32 | n_ok   (one add covers both; M < 2^31)
//   word 2  two u32: [0] the lowest non-OK row, [1] the lowest first_ne hit row,
//           kGatherNoRow when there is none
//   word 3  spare (0)
// The finish kernel resolves the outputs and writes the identities back, so a reduce
// always starts from the image the constructor wrote: no fill launch per reduce.
#pragma once
#include <stdint.h>

namespace ptype {

constexpr int kGatherSum = 0;
constexpr int kGatherMin = 1;
constexpr int kGatherMax = 2;
constexpr int kGatherFirstNe = 3;
constexpr int kGatherOps = 4;

constexpr int kGatherAccWords = 4;
constexpr uint32_t kGatherNoRow = 0xffffffffu;
// G <= kGatherLdsGroups: a block accumulates in LDS (24 B per group: 48 KiB, two
// blocks per CU fit in 160 KiB) and flushes every touched group once
constexpr int kGatherLdsGroups = 2048;
constexpr int64_t kGatherMaxGroups = 1ll << 26;
// blocks per launch (they stride over the tiles).  With the LDS arrays: at most two per
// CU, and no more than leave every block kGatherFlushRatio * G messages (each block
// flushes up to G groups: with 512 blocks of 2048 messages, G = 1024 random ids cost
// as many global atomics as messages and 1 Mi messages took 1.6 times as long as with
// 128 blocks, profiles/gather.md), but at least kGatherBlocksLdsMin.  Without them more, to keep atomics
// to HBM in flight.
constexpr int kGatherBlocksLds = 512;
constexpr int kGatherBlocksLdsMin = 64;
constexpr int kGatherFlushRatio = 8;
constexpr int kGatherBlocksHbm = 2048;

}  // namespace ptype
