// The topic records' parse and flatten (csrc/core/topic_follower.hpp) on a hostile corpus
// and a few thousand generated records, as a host program of its own so that
// AddressSanitizer + UBSan own the process (tests/test_topics_native.py builds and runs it).
// Every flattened table is checked against the records it was given: the arrays' shape,
// the counters, and a re-expansion of the accepted records.
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

std::string seg_json(const std::vector<TopicSegment>& segs) {
  std::string s = "{\"segments\": [";
  for (size_t i = 0; i < segs.size(); ++i) {
    if (i) s += ", ";
    s += "[" + std::to_string(segs[i].start) + ", " + std::to_string(segs[i].count) + ", " +
         std::to_string(segs[i].stride) + "]";
  }
  return s + "]}";
}

bool valid(const TopicSegment& s) {
  if (s.start < 0 || s.count < 1 || s.stride < 1) return false;
  const __int128 last = (__int128)s.start + (__int128)s.stride * (s.count - 1);
  return last <= (__int128)kTopicMaxActor;
}

// The table's invariants, whatever went in.
void check_table(const TopicFlat& t, int64_t max_topics, int64_t records) {
  CHECK((int64_t)t.seg_off.size() == max_topics + 1);
  CHECK(t.records == records);
  CHECK(t.bad_records >= 0 && t.bad_records <= t.records);
  const int64_t S = t.segments();
  CHECK((int64_t)t.row_off.size() == S + 1 && (int64_t)t.seg_stride.size() == S);
  CHECK(t.seg_off.front() == 0 && t.seg_off.back() == S && t.row_off.front() == 0);
  for (size_t g = 0; g + 1 < t.seg_off.size(); ++g) CHECK(t.seg_off[g] <= t.seg_off[g + 1]);
  int64_t in_subs = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t count = t.row_off[(size_t)s + 1] - t.row_off[(size_t)s];
    CHECK(valid(TopicSegment{t.seg_start[(size_t)s], count, t.seg_stride[(size_t)s]}));
  }
  int64_t prev_topic = -1;
  for (const TopicSub& u : t.subs) {
    CHECK(u.topic >= prev_topic && u.topic < max_topics && u.seg == in_subs && u.n_segs >= 1);
    CHECK(u.seg >= t.seg_off[(size_t)u.topic] && u.seg + u.n_segs <= t.seg_off[(size_t)u.topic + 1]);
    prev_topic = u.topic;
    in_subs += u.n_segs;
  }
  CHECK(in_subs == S);
  CHECK((int64_t)t.subs.size() == t.records - t.bad_records);
}

void hostile() {
  const std::string good = "{\"segments\": [[1, 2, 3]]}";
  const std::vector<std::pair<std::string, std::string>> corpus = {
      {"4/a", ""},
      {"4/a", "{"},
      {"4/a", "{\"segments\": [[1, 2, 3]"},
      {"4/a", "{\"segments\": [[1, 2, 3]]"},
      {"4/a", "[[1, 2, 3]]"},
      {"4/a", "null"},
      {"4/a", "{\"segments\": null}"},
      {"4/a", "{\"segments\": {}}"},
      {"4/a", "{\"segments\": []}"},
      {"4/a", "{\"segments\": [1, 2, 3]}"},
      {"4/a", "{\"segments\": [[1, 0, 1]]}"},
      {"4/a", "{\"segments\": [[1, 2, 0]]}"},
      {"4/a", "{\"segments\": [[-1, 2, 1]]}"},
      {"4/a", "{\"segments\": [[1, -2, 1]]}"},
      {"4/a", "{\"segments\": [[2147483646, 2, 1]]}"},
      {"4/a", "{\"segments\": [[2147483647, 1, 1]]}"},
      {"4/a", "{\"segments\": [[1, 3, 1073741824]]}"},
      {"4/a", "{\"segments\": [[0, 2147483648, 2147483648]]}"},
      {"4/a", "{\"segments\": [[0, 9223372036854775807, 9223372036854775807]]}"},
      {"4/a", "{\"segments\": [[1, 99999999999999999999999, 1]]}"},
      {"4/a", "{\"segments\": [[1, -99999999999999999999999, 1]]}"},
      {"4/a", "{\"segments\": [[1, 2.5, 1]]}"},
      {"4/a", "{\"segments\": [[1, 1e3, 1]]}"},
      {"4/a", "{\"segments\": [[\"1\", 2, 1]]}"},
      {"4/a", "{\"segments\": [[1, 2]]}"},
      {"4/a", "{\"segments\": [[1, 2, 1, 1]]}"},
      {"4/a", "{\"segments\": [[1, 2, 1], 7]}"},
      {"4/a", "{\"segments\": [[--, 2, 1]]}"},
      {"4/a", "{\"segments\": \"\\u00"},
      {"4/a", "{\"segments\": \"\\"},
      {"4/a", std::string("{\"segments\": [[1, 2, 3]]}\0trailing", 34)},
      {"4/a", std::string(100000, '[')},
      {"4/a", std::string(100000, '{')},
      {"4/a", "{\"segments\": " + std::string(50000, '[') + std::string(50000, ']') + "}"},
      {"4/a", "{\"segments\": [[1, 2, 3]], \"pad\": \"" + std::string(1u << 18, 'x') + "\"}"},
      {"8/a", good},
      {"99999999999999999999/a", good},
      {"1048576/a", good},
      {"four/a", good},
      {"-1/a", good},
      {"+4/a", good},
      {"04/a", good},
      {" 4/a", good},
      {"4 /a", good},
      {"4/", good},
      {"/a", good},
      {"4", good},
      {"", good},
      {"/", good},
  };
  const std::map<std::string, std::string> neighbours = {
      {"3/z", "{\"segments\": [[10, 2, 5]]}"}, {"4/0", "{\"segments\": [[1, 1, 1]]}"},
      {"4/z", "{\"segments\": [[7, 3, 1]]}"}, {"5/a", "{\"segments\": [[0, 2, 2]]}"}};
  const TopicFlat want = topics_flatten(neighbours, 8);
  CHECK(want.bad_records == 0 && want.segments() == 4 && want.subscribers() == 8 && want.topics == 3);
  for (const auto& kv : corpus) {
    std::map<std::string, std::string> recs = neighbours;
    recs[kv.first] = kv.second;
    const TopicFlat t = topics_flatten(recs, 8);
    check_table(t, 8, 5);
    const bool trailing = kv.second.size() == 34;  // (bytes after the value: the parser's leniency, either way)
    if (!trailing) CHECK(t.bad_records == 1);
    if (t.bad_records == 1) {
      CHECK(t.seg_off == want.seg_off && t.row_off == want.row_off && t.seg_start == want.seg_start &&
            t.seg_stride == want.seg_stride);
    }
  }
  // 1025 segments: refused; 1024: taken
  std::vector<TopicSegment> many(1025, TopicSegment{3, 1, 1});
  std::map<std::string, std::string> recs = neighbours;
  recs["4/many"] = seg_json(many);
  CHECK(topics_flatten(recs, 8).bad_records == 1);
  many.pop_back();
  recs["4/many"] = seg_json(many);
  const TopicFlat t = topics_flatten(recs, 8);
  CHECK(t.bad_records == 0 && t.segments() == 4 + 1024);
  check_table(t, 8, 5);
  for (int64_t bad : {(int64_t)0, (int64_t)-1, kTopicMaxTopics + 1}) {
    bool threw = false;
    try {
      topics_flatten(neighbours, bad);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
  }
  std::printf("OK hostile\n");
}

// A few thousand records, a third of them broken one way or another: the flatten accepts
// exactly the valid ones, in key order per topic, and expands to what the records say.
void generated(uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  const int64_t max_topics = 97;
  std::map<std::string, std::string> recs;
  std::map<std::string, std::vector<TopicSegment>> accepted;  // key -> segments
  for (int i = 0; i < 4000; ++i) {
    const int64_t topic = pick(0, 120);
    const std::string key = std::to_string(topic) + "/n" + std::to_string(pick(0, 60));
    std::vector<TopicSegment> segs;
    const int64_t n = pick(0, 12) == 0 ? pick(1020, 1030) : pick(0, 6);
    bool ok = topic < max_topics && n >= 1 && n <= kTopicMaxSegmentsPerRecord;
    for (int64_t j = 0; j < n; ++j) {
      TopicSegment s;
      switch (pick(0, 9)) {
        case 0: s = TopicSegment{pick(-3, 3), pick(-1, 3), pick(-1, 3)}; break;
        case 1: s = TopicSegment{kTopicMaxActor - pick(0, 40), pick(1, 5), pick(1, 12)}; break;
        case 2: {
          const int64_t c = pick(2, 1 << 20), st = kTopicMaxActor / (c - 1);
          s = TopicSegment{kTopicMaxActor - st * (c - 1) + pick(0, 1), c, st};
          break;
        }
        default: s = TopicSegment{pick(0, 1 << 24), pick(1, 1 << 16), pick(1, 64)};
      }
      ok = ok && valid(s);
      segs.push_back(s);
    }
    std::string value = seg_json(segs);
    if (pick(0, 40) == 0) {
      value.resize(value.size() / 2);  // torn
      ok = false;
    }
    recs[key] = value;
    if (ok)
      accepted[key] = segs;
    else
      accepted.erase(key);
  }
  const TopicFlat t = topics_flatten(recs, max_topics);
  check_table(t, max_topics, (int64_t)recs.size());
  CHECK((int64_t)t.subs.size() == (int64_t)accepted.size());
  // every accepted record, at its place: the subs of a topic are in key order
  std::map<int64_t, std::vector<std::string>> by_topic;
  for (const auto& kv : accepted) by_topic[std::stoll(kv.first.substr(0, kv.first.find('/')))].push_back(kv.first);
  size_t u = 0;
  int64_t with_subscriber = 0;
  for (const auto& tk : by_topic) {
    ++with_subscriber;
    for (const std::string& key : tk.second) {
      if (u >= t.subs.size()) {
        CHECK(false);
        break;
      }
      const TopicSub& sub = t.subs[u++];
      const auto& segs = accepted[key];
      CHECK(sub.topic == tk.first && sub.name == key.substr(key.find('/') + 1) && sub.n_segs == (int64_t)segs.size());
      for (int64_t j = 0; j < sub.n_segs && j < (int64_t)segs.size(); ++j) {
        const size_t s = (size_t)(sub.seg + j);
        CHECK(t.seg_start[s] == segs[(size_t)j].start && t.seg_stride[s] == segs[(size_t)j].stride &&
              t.row_off[s + 1] - t.row_off[s] == segs[(size_t)j].count);
      }
    }
  }
  CHECK(t.topics == with_subscriber);
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
  std::printf("OK topics_parse\n");
  return 0;
}
