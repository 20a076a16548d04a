// The control side of the pub/sub topic table (ops/topics.py), compiled: it follows a
// service's subscription records in the replicated store and flattens them into the four
// arrays the scatter's `topics` rule reads (csrc/hip/scatter.hpp).
//
// Record: `store/_ptype/topics/<service>/<topic>/<name>` ->
//   {"segments": [[start, count, stride], ...], "queue": true}
// `topic` is a decimal integer in [0, max_topics), `name` the subscription's name.  Segment
// s stands for the actor ids start + stride * k, 0 <= k < count; valid when count >= 1,
// stride >= 1, start >= 0 and start + stride * (count - 1) <= 2^31 - 2; a record holds 1 to
// 1024 segments.  A topic's subscribers are its records in key order, segments in record
// order; nothing is de-duplicated across records.  A record that is not valid (bad JSON, a
// field out of range, too many segments, a topic outside [0, max_topics), a table past
// 2^24 segments) is skipped and counted, never an error.
//
// `queue` is optional: absent or false is an ordinary subscription (every member gets every
// publication).  true makes the record a queue subscription -- a publication reaches exactly
// one of its members, the ids of its segments in record order; their number lies in
// [1, 2^31 - 1].  Any other value of `queue` makes the record invalid.  The queue segments
// follow the ordinary ones in row_off / seg_start / seg_stride (seg_off[max_topics] keeps
// bounding the ordinary ones); q_off maps a topic to its queue subscriptions (key order),
// q_seg a queue subscription to its first segment.  Ordinary plus queue segments and the
// queue subscriptions are at most 2^24 each; a record past a limit is skipped and counted.
// For records without a queue subscription the four ordinary arrays are what they always were.
//
// topics_flatten() is the pure part -- records in, arrays out, no thread, no KvClient.
// TopicFollower keeps the prefix's records current like RegistryFollower keeps the shard
// records: an initial list, a watch from the list's revision + 1, a periodic re-list as the
// backstop of a cancelled or compacted watch.  Subscriptions carry no deadline of their
// own (an ephemeral one is deleted by the store when its lease lapses), so quiet() is two
// loads: the version the watch thread bumps against the one take() applied.
#pragma once
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kvclient.hpp"
#include "util.hpp"

namespace ptype {

constexpr int64_t kTopicMaxSegmentsPerRecord = 1024;
constexpr int64_t kTopicMaxActor = 0x7ffffffell;      // 2^31 - 2
constexpr int64_t kTopicMaxSegments = 1ll << 24;      // of one table (scatter.hpp kScatterMaxSegments)
constexpr int64_t kTopicMaxTopics = 1ll << 20;        // gpu.topics
constexpr int64_t kTopicMaxQueues = 1ll << 24;        // queue subscriptions of one table
constexpr int64_t kTopicMaxQueueMembers = 0x7fffffffll;  // of one queue subscription: 2^31 - 1

struct TopicSegment {
  int64_t start = 0, count = 0, stride = 0;
};

// One accepted record of the flattened table: its segments are [seg, seg + n_segs).
struct TopicSub {
  int64_t topic = 0;
  std::string name;
  int64_t seg = 0, n_segs = 0;
};

struct TopicFlat {
  std::vector<int64_t> seg_off;     // [max_topics + 1]
  std::vector<int64_t> row_off;     // [S + 1]: the ordinary segments, then the queue segments
  std::vector<int32_t> seg_start;   // [S]
  std::vector<int32_t> seg_stride;  // [S]
  std::vector<int64_t> q_off;       // [max_topics + 1]: topic -> its queue subscriptions
  std::vector<int64_t> q_seg;       // [NQ + 1]: queue subscription -> its first segment; q_seg[0] = segments()
  std::vector<TopicSub> subs;       // the ordinary subscriptions: by topic, then key order
  std::vector<TopicSub> queues;     // the queue subscriptions, likewise
  int64_t records = 0, bad_records = 0;
  int64_t topics = 0;               // topics with an ordinary subscriber
  // of the ordinary subscriptions
  int64_t segments() const { return seg_off.empty() ? 0 : seg_off.back(); }
  int64_t subscribers() const { return row_off.empty() ? 0 : row_off[(size_t)segments()]; }
  // of the queue subscriptions
  int64_t queue_segments() const { return (int64_t)seg_start.size() - segments(); }
  int64_t queue_members() const { return row_off.empty() ? 0 : row_off.back() - subscribers(); }
};

// The segments of a record's value and whether it is a queue subscription; false when it
// is not a valid record.
bool topic_parse_record(const std::string& json, std::vector<TopicSegment>* out, bool* queue);
// (the segments alone: a queue record is a valid record)
bool topic_parse_record(const std::string& json, std::vector<TopicSegment>* out);
// "<topic>/<name>" (a key below the service's prefix); false when it names no topic of [0, max_topics).
bool topic_parse_key(const std::string& rest, int64_t max_topics, int64_t* topic, std::string* name);
// Records (key below the prefix -> value, in key order) into the table.
TopicFlat topics_flatten(const std::map<std::string, std::string>& records, int64_t max_topics);

class TopicFollower {
 public:
  // prefix: `store/_ptype/topics/<service>/`; relist_s: the re-list period; watch=false: re-list only.
  TopicFollower(std::shared_ptr<KvClient> kv, const std::string& prefix, int64_t max_topics, double relist_s,
                bool watch);
  ~TopicFollower();
  TopicFollower(const TopicFollower&) = delete;
  TopicFollower& operator=(const TopicFollower&) = delete;
  void close();

  bool quiet() const { return version_.load(std::memory_order_acquire) == applied_.load(std::memory_order_relaxed); }
  // The table of the records as they stand, and the store revision it reflects.
  TopicFlat take(int64_t* rev);
  // The store revision the records reflect.  Read it, then quiet(): when quiet() holds the
  // table of the last take() reflects that revision (versions move under the records' lock).
  int64_t rev() const;
  // Sleep until the watch thread saw an event or re-listed, or the timeout passed.
  void wait_change(int64_t timeout_ms);

  uint64_t version() const { return version_.load(std::memory_order_acquire); }
  uint64_t relists() const { return relists_.load(); }
  uint64_t events() const { return events_.load(); }
  int64_t max_topics() const { return max_topics_; }

 private:
  void run();
  void relist();

  std::shared_ptr<KvClient> kv_;
  std::string prefix_, end_;
  int64_t max_topics_;
  double relist_s_;
  Ctx ctx_;
  std::shared_ptr<Channel<WatchResponse>> watch_;
  std::thread th_;
  std::atomic<bool> stop_{false};
  bool watching_ = false;

  mutable std::mutex mu_;                       // records_, rev_ (watch thread vs take)
  std::condition_variable cv_;
  std::map<std::string, std::string> records_;  // key below the prefix -> value
  int64_t rev_ = 0;                             // the store revision records_ reflects
  int64_t list_rev_ = 0;                        // the revision of the last listing taken over
  std::atomic<uint64_t> version_{0}, applied_{~0ull};
  std::atomic<uint64_t> relists_{0}, events_{0};
};

}  // namespace ptype
