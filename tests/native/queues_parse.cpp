// The topic records' `queue` field (csrc/core/topic_follower.hpp) on a hostile corpus and a
// few thousand generated mixed record sets, as a host program of its own so that
// AddressSanitizer + UBSan own the process (tests/test_queues_native.py builds and runs it).
// Every flattened table is checked for the prefix property -- the four ordinary arrays and
// `subs` equal those of the same records without the queue records -- and for the internal
// consistency of q_off, q_seg and `queues`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "topic_follower.hpp"

using namespace ptype;

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

std::string seg_json(const std::vector<TopicSegment>& segs, const std::string& queue) {
  std::string s = "{\"segments\": [";
  for (size_t i = 0; i < segs.size(); ++i) {
    if (i) s += ", ";
    s += "[" + std::to_string(segs[i].start) + ", " + std::to_string(segs[i].count) + ", " +
         std::to_string(segs[i].stride) + "]";
  }
  s += "]";
  if (!queue.empty()) s += ", \"queue\": " + queue;
  return s + "}";
}

bool valid(const TopicSegment& s) {
  if (s.start < 0 || s.count < 1 || s.stride < 1) return false;
  const __int128 last = (__int128)s.start + (__int128)s.stride * (s.count - 1);
  return last <= (__int128)kTopicMaxActor;
}

bool same_subs(const std::vector<TopicSub>& a, const std::vector<TopicSub>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].topic != b[i].topic || a[i].name != b[i].name || a[i].seg != b[i].seg || a[i].n_segs != b[i].n_segs)
      return false;
  return true;
}

// The queue arrays' invariants, whatever went in.
void check_queues(const TopicFlat& t, int64_t max_topics) {
  const int64_t S = (int64_t)t.seg_start.size(), So = t.segments(), NQ = (int64_t)t.queues.size();
  CHECK((int64_t)t.seg_off.size() == max_topics + 1 && (int64_t)t.q_off.size() == max_topics + 1);
  CHECK((int64_t)t.row_off.size() == S + 1 && (int64_t)t.seg_stride.size() == S && (int64_t)t.q_seg.size() == NQ + 1);
  CHECK(So >= 0 && So <= S && S <= kTopicMaxSegments && NQ <= kTopicMaxQueues);
  CHECK(t.seg_off.front() == 0 && t.seg_off.back() == So && t.q_off.front() == 0 && t.q_off.back() == NQ);
  CHECK(t.q_seg.front() == So && t.q_seg.back() == S && t.row_off.front() == 0);
  CHECK(t.queue_segments() == S - So && t.subscribers() == t.row_off[(size_t)So]);
  CHECK(t.queue_members() == t.row_off.back() - t.row_off[(size_t)So]);
  for (size_t g = 0; g + 1 < t.q_off.size(); ++g) CHECK(t.q_off[g] <= t.q_off[g + 1] && t.seg_off[g] <= t.seg_off[g + 1]);
  for (int64_t s = 0; s < S; ++s) {
    const int64_t count = t.row_off[(size_t)s + 1] - t.row_off[(size_t)s];
    CHECK(valid(TopicSegment{t.seg_start[(size_t)s], count, t.seg_stride[(size_t)s]}));
  }
  int64_t prev_topic = -1;
  std::string prev_name;
  for (int64_t j = 0; j < NQ; ++j) {
    const TopicSub& u = t.queues[(size_t)j];
    const int64_t a = t.q_seg[(size_t)j], b = t.q_seg[(size_t)j + 1];
    CHECK(u.seg == a && u.n_segs == b - a && b - a >= 1 && b - a <= kTopicMaxSegmentsPerRecord);
    CHECK(u.topic >= 0 && u.topic < max_topics);
    CHECK(u.topic > prev_topic || (u.topic == prev_topic && u.name > prev_name));  // by topic, then key order
    if (u.topic >= 0 && u.topic < max_topics) CHECK(j >= t.q_off[(size_t)u.topic] && j < t.q_off[(size_t)u.topic + 1]);
    const int64_t members = t.row_off[(size_t)b] - t.row_off[(size_t)a];
    CHECK(members >= 1 && members <= kTopicMaxQueueMembers);
    prev_topic = u.topic, prev_name = u.name;
  }
  CHECK((int64_t)(t.subs.size() + t.queues.size()) == t.records - t.bad_records);
}

// The prefix property: `all` flattened against the same records without the queue records.
void check_prefix(const TopicFlat& all, const TopicFlat& plain) {
  const size_t So = (size_t)plain.seg_start.size();
  CHECK(plain.queues.empty() && plain.q_seg.size() == 1 && plain.q_seg[0] == (int64_t)So);
  CHECK(all.seg_off == plain.seg_off && same_subs(all.subs, plain.subs) && all.topics == plain.topics);
  CHECK(all.segments() == plain.segments() && all.subscribers() == plain.subscribers());
  CHECK(all.row_off.size() >= So + 1 && all.seg_start.size() >= So);
  if (all.row_off.size() >= So + 1 && all.seg_start.size() >= So) {
    CHECK(std::vector<int64_t>(all.row_off.begin(), all.row_off.begin() + (long)So + 1) == plain.row_off);
    CHECK(std::vector<int32_t>(all.seg_start.begin(), all.seg_start.begin() + (long)So) == plain.seg_start);
    CHECK(std::vector<int32_t>(all.seg_stride.begin(), all.seg_stride.begin() + (long)So) == plain.seg_stride);
  }
}

void hostile() {
  const std::string seg = "\"segments\": [[1, 2, 3]]";
  const std::vector<std::string> bad_values = {
      "1", "0", "-1", "1.0", "1e0", "\"true\"", "\"\"", "null", "[]", "[true]", "{}", "{\"queue\": true}", "tru", "TRUE",
      "True", "truee", "", "99999999999999999999999", "\"\\u00", std::string(100000, '['),
  };
  const std::map<std::string, std::string> neighbours = {
      {"3/z", "{\"segments\": [[10, 2, 5]]}"}, {"4/0", "{\"segments\": [[1, 1, 1]], \"queue\": true}"},
      {"4/z", "{\"segments\": [[7, 3, 1]]}"}, {"5/a", "{\"queue\": true, \"segments\": [[0, 2, 2], [9, 9, 9]]}"}};
  const TopicFlat want = topics_flatten(neighbours, 8);
  check_queues(want, 8);
  CHECK(want.bad_records == 0 && want.segments() == 2 && want.subscribers() == 5 && want.topics == 2);
  CHECK(want.queues.size() == 2 && want.queue_segments() == 3 && want.queue_members() == 12);
  CHECK(want.q_off == (std::vector<int64_t>{0, 0, 0, 0, 0, 1, 2, 2, 2}) && want.q_seg == (std::vector<int64_t>{2, 3, 5}));
  for (const std::string& v : bad_values) {
    for (const std::string& value : {"{" + seg + ", \"queue\": " + v + "}", "{\"queue\": " + v + ", " + seg + "}"}) {
      std::map<std::string, std::string> recs = neighbours;
      recs["4/a"] = value;
      const TopicFlat t = topics_flatten(recs, 8);
      check_queues(t, 8);
      CHECK(t.records == 5 && t.bad_records == 1);
      CHECK(t.seg_off == want.seg_off && t.row_off == want.row_off && t.seg_start == want.seg_start &&
            t.seg_stride == want.seg_stride && t.q_off == want.q_off && t.q_seg == want.q_seg);
      CHECK(same_subs(t.subs, want.subs) && same_subs(t.queues, want.queues));
    }
  }
  // the values that are taken: true, false, absent, spaces
  std::vector<TopicSegment> out;
  bool queue = false;
  CHECK(topic_parse_record("{" + seg + ", \"queue\": true}", &out, &queue) && queue && out.size() == 1);
  CHECK(topic_parse_record("{" + seg + ", \"queue\": false}", &out, &queue) && !queue);
  CHECK(topic_parse_record("{" + seg + "}", &out, &queue) && !queue);
  CHECK(topic_parse_record(" { \"queue\" : true , " + seg + " } ", &out, &queue) && queue);
  CHECK(topic_parse_record("{" + seg + ", \"queue\": true}", &out) && out.size() == 1);
  CHECK(!topic_parse_record("{" + seg + ", \"queue\": 1}", &out, &queue) && !queue && out.empty());
  // the member count of a queue subscription: 2^31 - 1 is taken, 2^31 is not; an ordinary record may hold more
  const int64_t big = kTopicMaxQueueMembers;
  CHECK(topic_parse_record(seg_json({{0, big, 1}}, "true"), &out, &queue) && queue);
  CHECK(topic_parse_record(seg_json({{0, big - 1, 1}, {7, 1, 1}}, "true"), &out, &queue) && queue);
  CHECK(!topic_parse_record(seg_json({{0, big, 1}, {7, 1, 1}}, "true"), &out, &queue));
  CHECK(topic_parse_record(seg_json({{0, big, 1}, {7, 1, 1}}, "false"), &out, &queue) && !queue);
  CHECK(topic_parse_record(seg_json(std::vector<TopicSegment>(1024, TopicSegment{0, big, 1}), ""), &out, &queue) && !queue);
  CHECK(!topic_parse_record(seg_json(std::vector<TopicSegment>(1024, TopicSegment{0, big, 1}), "true"), &out, &queue));
  // 1025 segments: refused; 1024: taken
  std::vector<TopicSegment> many(1025, TopicSegment{3, 1, 1});
  std::map<std::string, std::string> recs = neighbours;
  recs["4/many"] = seg_json(many, "true");
  CHECK(topics_flatten(recs, 8).bad_records == 1);
  many.pop_back();
  recs["4/many"] = seg_json(many, "true");
  const TopicFlat t = topics_flatten(recs, 8);
  CHECK(t.bad_records == 0 && t.segments() == 2 && t.queue_segments() == 3 + 1024 && t.queues.size() == 3);
  check_queues(t, 8);
  std::printf("OK hostile\n");
}

// A few thousand records, ordinary and queue, a third of them broken one way or another.
void generated(uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  const int64_t max_topics = 97;
  std::map<std::string, std::string> recs, plain_recs;
  std::map<std::string, std::vector<TopicSegment>> accepted_q;  // key -> segments of the accepted queue records
  const std::vector<std::string> odd = {"1", "null", "\"true\"", "[true]", "0.5"};
  for (int i = 0; i < 4000; ++i) {
    const int64_t topic = pick(0, 120);
    const std::string key = std::to_string(topic) + "/n" + std::to_string(pick(0, 60));
    std::vector<TopicSegment> segs;
    const int64_t n = pick(0, 12) == 0 ? pick(1020, 1030) : pick(0, 6);
    bool ok = topic < max_topics && n >= 1 && n <= kTopicMaxSegmentsPerRecord;
    __int128 members = 0;
    for (int64_t j = 0; j < n; ++j) {
      TopicSegment s;
      switch (pick(0, 9)) {
        case 0: s = TopicSegment{pick(-3, 3), pick(-1, 3), pick(-1, 3)}; break;
        case 1: s = TopicSegment{kTopicMaxActor - pick(0, 40), pick(1, 5), pick(1, 12)}; break;
        case 2: s = TopicSegment{pick(0, 5), kTopicMaxQueueMembers / pick(1, 3) - pick(0, 5), 1}; break;
        default: s = TopicSegment{pick(0, 1 << 24), pick(1, 1 << 16), pick(1, 64)};
      }
      ok = ok && valid(s);
      members += s.count;
      segs.push_back(s);
    }
    const int64_t kind = pick(0, 9);  // 0-3 absent, 4 false, 5-8 true, 9 something else
    const bool queue = kind >= 5 && kind <= 8;
    std::string value = seg_json(segs, kind <= 3 ? "" : kind == 4 ? "false" : queue ? "true" : odd[(size_t)pick(0, 4)]);
    if (kind == 9) ok = false;
    if (queue && members > (__int128)kTopicMaxQueueMembers) ok = false;
    if (pick(0, 40) == 0) {
      value.resize(value.size() / 2);  // torn
      ok = false;
    }
    recs[key] = value;
    accepted_q.erase(key);
    plain_recs.erase(key);
    if (ok && queue) accepted_q[key] = segs;
    if (!queue) plain_recs[key] = value;
  }
  const TopicFlat t = topics_flatten(recs, max_topics);
  check_queues(t, max_topics);
  CHECK(t.records == (int64_t)recs.size());
  const TopicFlat plain = topics_flatten(plain_recs, max_topics);
  check_queues(plain, max_topics);
  check_prefix(t, plain);
  CHECK(t.bad_records - plain.bad_records == (int64_t)(recs.size() - plain_recs.size()) - (int64_t)accepted_q.size());
  // every accepted queue record, at its place and with its segments
  CHECK(t.queues.size() == accepted_q.size());
  std::map<int64_t, std::vector<std::string>> by_topic;
  for (const auto& kv : accepted_q) by_topic[std::stoll(kv.first.substr(0, kv.first.find('/')))].push_back(kv.first);
  size_t u = 0;
  for (const auto& tk : by_topic) {
    for (const std::string& key : tk.second) {
      if (u >= t.queues.size()) {
        CHECK(false);
        break;
      }
      const TopicSub& sub = t.queues[u++];
      const auto& segs = accepted_q[key];
      CHECK(sub.topic == tk.first && sub.name == key.substr(key.find('/') + 1) && sub.n_segs == (int64_t)segs.size());
      for (int64_t j = 0; j < sub.n_segs && j < (int64_t)segs.size(); ++j) {
        const size_t s = (size_t)(sub.seg + j);
        CHECK(t.seg_start[s] == segs[(size_t)j].start && t.seg_stride[s] == segs[(size_t)j].stride &&
              t.row_off[s + 1] - t.row_off[s] == segs[(size_t)j].count);
      }
    }
  }
}

}  // namespace

int main() {
  hostile();
  for (uint64_t seed = 1; seed <= 3; ++seed) generated(seed);
  std::printf("OK generated\n");
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("OK queues_parse\n");
  return 0;
}
