// Tile shape and size limits of the counting sorts, free of HIP: what the host-side
// plan of a mailbox Send (mailbox_plan.hpp) and the device code both read.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ptype {

// 512 threads (8 waves) per block, 4096-message tiles: with 256 shards a tile
// gives each shard a run of ~16 records (256 B, two whole lines) instead of ~8
// -- half-written lines evicted from L2 before their other half arrived made
// the 2048-message tiles write 1.9x the record bytes (PMC, r3).
constexpr int kST = 512;                 // count / scatter threads per block
constexpr int kSK = 8;                   // messages per thread per tile
constexpr int kSTile = kST * kSK;        // 4096 messages

constexpr uint32_t kMaxMbox = 1u << 24;

// Sorted epoch mailboxes (mailbox_sort.hip): shard limit, and the per-(block,
// shard) histogram's size -- it bounds the count / scatter grid (G <= words / S)
constexpr int kMboxSortMaxShards = 1024;
constexpr uint32_t kMboxSortHistWords = 1u << 18;
constexpr uint32_t kMboxSortGroups = 32;  // group sums of 32 blocks each (G <= 1024)
constexpr uint32_t kGroupBlocks = 32;     // the scatter's prefix: group sums + rows inside the group

// Route mode 4's presence map: 2 bits per directory id, staged whole in LDS
constexpr uint32_t kPresMax = 1u << 18;  // ids (64 KB of map)
constexpr uint32_t pres_words(uint32_t n_dir) { return ((n_dir + 15) / 16 + 3) & ~3u; }
constexpr size_t kPresLdsMax = (size_t)pres_words(kPresMax) * 4;  // (past the 64 KB default dynamic LDS)

}  // namespace ptype
