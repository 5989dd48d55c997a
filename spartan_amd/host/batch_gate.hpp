// spartan_amd host driver: the rendezvous of SNARK::verify_many (verifier.cc). K members — one host thread per proof — run the same code over
// different data; where that code needs the device a member POSTS a request (a key and a payload) and blocks. When every member that is
// still inside has posted, one of them, the leader, hands the requests, grouped by key, to the function the gate was made with — one call
// per group — and gives every member its answer. So K requests of the same shape cost one device call, and the device sees one caller.
//
// Nothing here knows the device or the sp_* ABI (tests/csrc/gate_check.cc drives it with a stub under the thread and address sanitizers).
//
// Rules:
//   * a member is inside from the start; it leaves once, by leave() — GateMember does it on scope exit, so by return and by exception alike;
//   * a round runs when posted == inside and posted > 0. The member whose post() completes the set leads; when it is a leave() that
//     completes it, the leaving thread only wakes the waiters and the first of them to wake leads. No member waits on a condition that only
//     a departed member could make true: a waiter waits for "my answer is there OR the set is complete and nobody leads";
//   * while a round runs every member inside is blocked in post(), so the function runs alone: one leader at a time, no lock held;
//   * if the function throws, the round ends at once and EVERY member of the round — the groups already served included — gets that
//     exception out of post(). The gate is reset before they wake: members unwind through leave(), or post again;
//   * the function must return one answer per request of the group, in the order given; another count is a std::logic_error to the round.
#pragma once
#include <condition_variable>
#include <cstddef>
#include <exception>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <utility>
#include <vector>

namespace spz {

template <class Key /* operator< */, class Payload, class Answer>
class BatchGate {
 public:
  // serve one group: reqs[i] is the payload member `members[i]` posted under `key`; fill answers[i] for each
  typedef std::function<void(const Key& key, const std::vector<size_t>& members, const std::vector<const Payload*>& reqs, std::vector<Answer>& answers)> ServeFn;

  BatchGate(size_t members, ServeFn serve) : serve_(std::move(serve)), slots_(members), inside_(members) {}
  BatchGate(const BatchGate&) = delete;
  BatchGate& operator=(const BatchGate&) = delete;

  // member m posts and blocks for its answer; throws what the leader's function threw
  Answer post(size_t m, const Key& key, const Payload& payload) {
    std::unique_lock<std::mutex> lk(mu_);
    Slot& s = slots_.at(m);
    if (s.left || s.state != IDLE) throw std::logic_error("BatchGate::post: member has left or has a request pending");
    s.key = key;
    s.payload = &payload;
    s.state = POSTED;
    posted_++;
    for (;;) {
      if (s.state == DONE) break;
      if (posted_ == inside_ && !leading_) { lead(lk); continue; }
      cv_.wait(lk);
    }
    s.state = IDLE;
    if (s.error) {
      std::exception_ptr e = s.error;
      s.error = nullptr;
      std::rethrow_exception(e);
    }
    return std::move(s.answer);
  }

  // member m leaves for good (idempotent). If it was the one the others were waiting for, they are woken and one of them leads.
  void leave(size_t m) noexcept {
    std::lock_guard<std::mutex> lk(mu_);
    Slot& s = slots_[m];
    if (s.left) return;
    s.left = true;
    if (s.state == POSTED) posted_--;  // cannot happen through post(), which returns only with its answer; kept for a consistent count
    s.state = IDLE;
    inside_--;
    if (posted_ > 0 && posted_ == inside_) cv_.notify_all();
  }

  size_t inside() const {
    std::lock_guard<std::mutex> lk(mu_);
    return inside_;
  }
  size_t rounds() const {  // rendezvous served so far
    std::lock_guard<std::mutex> lk(mu_);
    return rounds_;
  }

 private:
  enum State { IDLE, POSTED, DONE };
  struct Slot {
    State state = IDLE;
    bool left = false;
    Key key{};
    const Payload* payload = nullptr;
    Answer answer{};
    std::exception_ptr error;
  };

  // called with the lock held by a member of a complete set; returns with the lock held and every posted slot DONE
  void lead(std::unique_lock<std::mutex>& lk) {
    leading_ = true;
    std::map<Key, std::vector<size_t>> groups;
    for (size_t i = 0; i < slots_.size(); i++)
      if (slots_[i].state == POSTED) groups[slots_[i].key].push_back(i);
    lk.unlock();  // everyone inside is blocked in post(): the slots do not change under the function
    std::exception_ptr err;
    std::vector<std::pair<size_t, Answer>> results;
    try {
      for (auto& g : groups) {
        std::vector<const Payload*> reqs;
        for (size_t i : g.second) reqs.push_back(slots_[i].payload);
        std::vector<Answer> answers;
        serve_(g.first, g.second, reqs, answers);
        if (answers.size() != reqs.size()) throw std::logic_error("BatchGate: the serving function returned another number of answers than requests");
        for (size_t k = 0; k < reqs.size(); k++) results.emplace_back(g.second[k], std::move(answers[k]));
      }
    } catch (...) {
      err = std::current_exception();
    }
    lk.lock();
    if (err) {
      for (Slot& s : slots_)
        if (s.state == POSTED) { s.error = err; s.state = DONE; }
    } else {
      for (auto& r : results) {
        Slot& s = slots_[r.first];
        s.answer = std::move(r.second);
        s.error = nullptr;
        s.state = DONE;
      }
    }
    posted_ = 0;
    rounds_++;
    leading_ = false;
    cv_.notify_all();
  }

  ServeFn serve_;
  mutable std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Slot> slots_;
  size_t inside_, posted_ = 0, rounds_ = 0;
  bool leading_ = false;
};

// a member's stay: leaves the gate on scope exit, however the scope is left
template <class Gate>
struct GateMember {
  Gate& gate;
  size_t m;
  GateMember(Gate& g, size_t m_) : gate(g), m(m_) {}
  ~GateMember() { gate.leave(m); }
  GateMember(const GateMember&) = delete;
  GateMember& operator=(const GateMember&) = delete;
};

}  // namespace spz
