// TopicFollower / topics_flatten (topic_follower.hpp).
#include "topic_follower.hpp"

#include <algorithm>
#include <chrono>

#include "json.hpp"

namespace ptype {

namespace {
std::string prefix_end(const std::string& p) {
  std::string e = p;
  e.back() = (char)(e.back() + 1);
  return e;
}

constexpr size_t kTopicMaxValueBytes = 1u << 17;  // 1024 segments of three 10-digit numbers fit in 40 KB
constexpr int kTopicMaxDepth = 8;                  // {"segments": [[..]]} nests three deep

// The JSON number at s[i..]: -?digits(.digits)?([eE][+-]?digits)?; returns its end, 0 when it is none.
size_t number_end(const std::string& s, size_t i) {
  auto digits = [&](size_t at) {
    while (at < s.size() && s[at] >= '0' && s[at] <= '9') ++at;
    return at;
  };
  if (i < s.size() && s[i] == '-') ++i;
  size_t e = digits(i);
  if (e == i) return 0;
  if (e < s.size() && s[e] == '.') {
    const size_t f = digits(e + 1);
    if (f == e + 1) return 0;
    e = f;
  }
  if (e < s.size() && (s[e] == 'e' || s[e] == 'E')) {
    size_t x = e + 1;
    if (x < s.size() && (s[x] == '+' || s[x] == '-')) ++x;
    const size_t f = digits(x);
    if (f == x) return 0;
    e = f;
  }
  return e;
}

// json_parse recurses per nesting level and takes any run of number characters for a
// number: a value from the store is bounded, and its numbers are checked, before it is parsed.
bool shallow(const std::string& s) {
  if (s.size() > kTopicMaxValueBytes) return false;
  int depth = 0;
  bool in_str = false;
  for (size_t i = 0; i < s.size(); ++i) {
    const char c = s[i];
    if (in_str) {
      if (c == '\\') ++i;
      else if (c == '"') in_str = false;
    } else if (c == '"') {
      in_str = true;
    } else if (c == '-' || c == '+' || c == '.' || (c >= '0' && c <= '9')) {
      const size_t e = number_end(s, i);
      if (!e) return false;
      i = e - 1;
    } else if (c == '[' || c == '{') {
      if (++depth > kTopicMaxDepth) return false;
    } else if (c == ']' || c == '}') {
      --depth;
    }
  }
  return true;
}
}  // namespace

bool topic_parse_record(const std::string& json, std::vector<TopicSegment>* out) {
  bool queue = false;
  return topic_parse_record(json, out, &queue);
}

bool topic_parse_record(const std::string& json, std::vector<TopicSegment>* out, bool* queue) {
  out->clear();
  *queue = false;
  if (!shallow(json)) return false;
  JValue v;
  try {
    v = json_parse(json);
  } catch (const std::exception&) {
    return false;
  }
  if (v.kind != JValue::kObject) return false;
  const JValue* segs = v.get("segments");
  if (!segs || segs->kind != JValue::kArray) return false;
  if (segs->arr.empty() || (int64_t)segs->arr.size() > kTopicMaxSegmentsPerRecord) return false;
  if (const JValue* q = v.get("queue")) {
    if (q->kind != JValue::kBool) return false;
    *queue = q->b;
  }
  int64_t members = 0;
  out->reserve(segs->arr.size());
  for (const JValue& s : segs->arr) {
    if (s.kind != JValue::kArray || s.arr.size() != 3) return false;
    for (const JValue& x : s.arr)
      if (x.kind != JValue::kNumber || !x.is_int) return false;
    TopicSegment t;
    t.start = (int64_t)s.arr[0].i, t.count = (int64_t)s.arr[1].i, t.stride = (int64_t)s.arr[2].i;
    // (every factor is bounded before the product: no overflow)
    if (t.start < 0 || t.start > kTopicMaxActor || t.count < 1 || t.count > kTopicMaxActor + 1 || t.stride < 1 ||
        t.stride > kTopicMaxActor)
      return false;
    if (t.count > 1 && t.stride > (kTopicMaxActor - t.start) / (t.count - 1)) return false;
    members += t.count;  // (1024 counts of at most 2^31 - 1)
    out->push_back(t);
  }
  if (*queue && members > kTopicMaxQueueMembers) return false;
  return true;
}

bool topic_parse_key(const std::string& rest, int64_t max_topics, int64_t* topic, std::string* name) {
  const size_t slash = rest.find('/');
  if (slash == std::string::npos || slash == 0 || slash > 7 || slash + 1 >= rest.size()) return false;
  int64_t g = 0;
  for (size_t i = 0; i < slash; ++i) {
    if (rest[i] < '0' || rest[i] > '9') return false;
    g = g * 10 + (rest[i] - '0');
  }
  if (slash > 1 && rest[0] == '0') return false;  // one spelling per topic
  if (g >= max_topics) return false;
  *topic = g;
  *name = rest.substr(slash + 1);
  return true;
}

TopicFlat topics_flatten(const std::map<std::string, std::string>& records, int64_t max_topics) {
  if (max_topics < 1 || max_topics > kTopicMaxTopics) throw std::invalid_argument("topics_flatten: max_topics must be in [1, 2^20]");
  TopicFlat t;
  struct Rec {
    int64_t topic;
    std::string name;
    std::vector<TopicSegment> segs;
    bool queue;
  };
  std::vector<Rec> good;
  std::vector<int64_t> per_topic((size_t)max_topics + 1, 0);   // ordinary segments of topic g at [g + 1]
  std::vector<int64_t> q_per_topic((size_t)max_topics + 1, 0);  // queue subscriptions of topic g at [g + 1]
  int64_t total = 0, ordinary = 0, n_queues = 0;
  for (const auto& kv : records) {
    ++t.records;
    Rec r;
    r.queue = false;
    if (!topic_parse_key(kv.first, max_topics, &r.topic, &r.name) || !topic_parse_record(kv.second, &r.segs, &r.queue) ||
        total + (int64_t)r.segs.size() > kTopicMaxSegments || (r.queue && n_queues + 1 > kTopicMaxQueues)) {
      ++t.bad_records;
      continue;
    }
    total += (int64_t)r.segs.size();
    if (r.queue) {
      ++n_queues;
      ++q_per_topic[(size_t)r.topic + 1];
    } else {
      ordinary += (int64_t)r.segs.size();
      per_topic[(size_t)r.topic + 1] += (int64_t)r.segs.size();
    }
    good.push_back(std::move(r));
  }
  // by topic; key order within a topic is the map's order, kept by the stable sort
  std::stable_sort(good.begin(), good.end(), [](const Rec& a, const Rec& b) { return a.topic < b.topic; });
  t.seg_off.assign((size_t)max_topics + 1, 0);
  t.q_off.assign((size_t)max_topics + 1, 0);
  for (int64_t g = 0; g < max_topics; ++g) {
    t.seg_off[(size_t)g + 1] = t.seg_off[(size_t)g] + per_topic[(size_t)g + 1];
    t.q_off[(size_t)g + 1] = t.q_off[(size_t)g] + q_per_topic[(size_t)g + 1];
    if (per_topic[(size_t)g + 1]) ++t.topics;
  }
  t.row_off.reserve((size_t)total + 1);
  t.seg_start.reserve((size_t)total);
  t.seg_stride.reserve((size_t)total);
  t.q_seg.reserve((size_t)n_queues + 1);
  t.row_off.push_back(0);
  // the ordinary subscriptions first, then the queue subscriptions: both by topic, then key order
  for (const bool queue : {false, true}) {
    if (queue) t.q_seg.push_back(ordinary);
    for (Rec& r : good) {
      if (r.queue != queue) continue;
      (queue ? t.queues : t.subs)
          .push_back(TopicSub{r.topic, std::move(r.name), (int64_t)t.seg_start.size(), (int64_t)r.segs.size()});
      for (const TopicSegment& s : r.segs) {
        t.seg_start.push_back((int32_t)s.start);
        t.seg_stride.push_back((int32_t)s.stride);
        t.row_off.push_back(t.row_off.back() + s.count);
      }
      if (queue) t.q_seg.push_back((int64_t)t.seg_start.size());
    }
  }
  return t;
}

// ---------------------------------------------------------------- TopicFollower
TopicFollower::TopicFollower(std::shared_ptr<KvClient> kv, const std::string& prefix, int64_t max_topics,
                             double relist_s, bool watch)
    : kv_(std::move(kv)), prefix_(prefix), end_(prefix.empty() ? prefix : prefix_end(prefix)), max_topics_(max_topics),
      relist_s_(relist_s) {
  if (prefix_.empty()) throw std::invalid_argument("TopicFollower: empty prefix");
  if (max_topics < 1 || max_topics > kTopicMaxTopics) throw std::invalid_argument("TopicFollower: max_topics must be in [1, 2^20]");
  RangeOpts o;
  o.end = end_;
  const RangeResult res = kv_->get(prefix_, o);
  {
    std::lock_guard<std::mutex> g(mu_);
    for (const auto& x : res.kvs) records_[x.key.substr(prefix_.size())] = x.value;
    rev_ = list_rev_ = res.rev;
  }
  version_.fetch_add(1, std::memory_order_release);
  ctx_ = Context::with_cancel(Context::background());
  watching_ = watch;
  if (watch) watch_ = kv_->watch(ctx_, prefix_, end_, res.rev + 1);
  th_ = std::thread([this] { run(); });
}

TopicFollower::~TopicFollower() { close(); }

void TopicFollower::close() {
  if (stop_.exchange(true)) return;
  if (ctx_) ctx_->cancel();
  if (th_.joinable()) th_.join();
  cv_.notify_all();
}

void TopicFollower::run() {
  const int64_t period_ms = std::max<int64_t>(1, (int64_t)(relist_s_ * 1000));
  auto next_list = std::chrono::steady_clock::now() + std::chrono::milliseconds(period_ms);
  const int64_t poll_ms = std::min<int64_t>(100, period_ms);
  while (!stop_.load()) {
    if (watch_ && !watch_->closed()) {
      bool closed = false;
      auto resp = watch_->recv(poll_ms, &closed);
      if (resp && !resp->events.empty()) {
        {
          std::lock_guard<std::mutex> g(mu_);
          for (const Event& ev : resp->events) {
            if (ev.kv.key.size() < prefix_.size()) continue;
            if (ev.kv.mod_revision <= list_rev_) continue;  // (a listing already holds what a late event says)
            const std::string rest = ev.kv.key.substr(prefix_.size());
            if (ev.type == Event::kPut)
              records_[rest] = ev.kv.value;
            else
              records_.erase(rest);
            rev_ = std::max(rev_, ev.kv.mod_revision);
            events_.fetch_add(1);
          }
          version_.fetch_add(1, std::memory_order_release);  // (under the lock: rev() then quiet() is consistent)
        }
        cv_.notify_all();
      }
    } else if (ctx_->wait(poll_ms)) {
      break;
    }
    if (std::chrono::steady_clock::now() >= next_list) {
      next_list = std::chrono::steady_clock::now() + std::chrono::milliseconds(period_ms);
      relist();
    }
  }
}

// A full re-list: what the watch missed (a closed or compacted watch, which is re-opened
// from just past the listing) shows up as a difference from the records kept.
void TopicFollower::relist() {
  RangeResult res;
  try {
    RangeOpts o;
    o.end = end_;
    res = kv_->get(prefix_, o, 2000);
  } catch (const std::exception&) {
    return;  // control plane electing: keep the last view
  }
  if (watching_ && watch_ && watch_->closed() && !stop_.load()) {
    try {
      watch_ = kv_->watch(ctx_, prefix_, end_, res.rev + 1);
    } catch (const std::exception&) {
    }
  }
  std::map<std::string, std::string> listed;
  for (const auto& x : res.kvs) listed[x.key.substr(prefix_.size())] = x.value;
  bool changed = false;
  {
    std::lock_guard<std::mutex> g(mu_);
    // (an event newer than the listing may already be applied: the listing is older, keep the records)
    if (res.rev >= rev_) {
      changed = listed != records_;
      if (changed) {
        records_.swap(listed);
        version_.fetch_add(1, std::memory_order_release);
      }
      rev_ = list_rev_ = res.rev;  // (the records reflect it, changed or not: no version moves for other prefixes' writes)
    }
  }
  relists_.fetch_add(1);
  cv_.notify_all();
}

TopicFlat TopicFollower::take(int64_t* rev) {
  std::map<std::string, std::string> records;
  uint64_t version;
  {
    std::lock_guard<std::mutex> g(mu_);
    records = records_;
    *rev = rev_;
    version = version_.load(std::memory_order_acquire);
  }
  TopicFlat t = topics_flatten(records, max_topics_);
  applied_.store(version, std::memory_order_relaxed);
  return t;
}

int64_t TopicFollower::rev() const {
  std::lock_guard<std::mutex> g(mu_);
  return rev_;
}

void TopicFollower::wait_change(int64_t timeout_ms) {
  std::unique_lock<std::mutex> g(mu_);
  cv_.wait_for(g, std::chrono::milliseconds(timeout_ms));  // (woken by every event and re-list)
}

}  // namespace ptype
