// Stand-alone check of spartan_amd/host/batch_gate.hpp (tests/test_verify_gate.py builds it with -fsanitize=thread and with
// -fsanitize=address,undefined and runs both under a time limit: a deadlock shows as the timeout). No device, no sp_* call: the "device" is
// a stub that answers f(key, payload) and keeps its books in PLAIN variables, so the thread sanitizer also checks that the gate runs it alone.
//
// K members walk through randomised numbers of steps with mixed keys (one rendezvous yields several groups), leave by return and by
// exception at every step position, and the stub throws on a chosen rendezvous. Checked: every request gets the answer computed from its own
// payload; the stub is invoked once per group and rendezvous; after a leader failure every member of that rendezvous sees the exception,
// and the gate goes on working for those that post again; the program ends.
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <thread>
#include <vector>

#include "../../spartan_amd/host/batch_gate.hpp"

namespace {
struct Key {
  int kind;
  size_t n;
  bool operator<(const Key& o) const { return kind != o.kind ? kind < o.kind : n < o.n; }
  bool operator==(const Key& o) const { return kind == o.kind && n == o.n; }
};
typedef spz::BatchGate<Key, uint64_t, uint64_t> Gate;
struct LeaderFail {};
struct Quit {};

uint64_t mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
  return x;
}
uint64_t f(const Key& k, uint64_t p) { return mix(p * 3 + (uint64_t)k.kind) + k.n; }
Key key_of(size_t m, int s) { return Key{(int)((m + (size_t)s) % 3), (size_t)32 << ((m * 7 + (size_t)s) % 2)}; }
uint64_t payload_of(uint64_t seed, size_t m, int s) { return mix(seed * 1000003 + m * 131 + (uint64_t)s); }

struct Plan { int steps; bool throws; };
int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { g_fail++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// one scenario. fail_round < 0: the stub never throws. resume: members that saw the leader's failure go on with their next step
void run(const std::vector<Plan>& plans, uint64_t seed, long fail_round, bool resume) {
  const size_t K = plans.size();
  // the stub's books: plain on purpose (see the head of the file)
  std::map<Key, long> calls;
  long invocations = 0;
  Gate* gp = nullptr;
  Gate gate(K, [&](const Key& key, const std::vector<size_t>& members, const std::vector<const uint64_t*>& reqs, std::vector<uint64_t>& answers) {
    invocations++;
    calls[key]++;
    if ((long)gp->rounds() == fail_round) throw LeaderFail();
    for (size_t i = 0; i < reqs.size(); i++) answers.push_back(f(key, *reqs[i]));
    (void)members;
  });
  gp = &gate;
  std::vector<int> wrong(K, 0), saw_fail(K, 0), done_steps(K, 0);
  std::vector<std::thread> th;
  for (size_t m = 0; m < K; m++)
    th.emplace_back([&, m]() {
      try {
        spz::GateMember<Gate> in(gate, m);
        for (int s = 0; s < plans[m].steps; s++) {
          const Key k = key_of(m, s);
          const uint64_t p = payload_of(seed, m, s);
          try {
            if (gate.post(m, k, p) != f(k, p)) wrong[m]++;
          } catch (const LeaderFail&) {
            saw_fail[m]++;
            if (!resume) throw;
          }
          done_steps[m]++;
        }
        if (plans[m].throws) throw Quit();
      } catch (const Quit&) {
      } catch (const LeaderFail&) {
      }
    });
  for (auto& t : th) t.join();

  // what must have happened, from the plans alone: rendezvous r gathers the members with more than r steps
  int max_steps = 0;
  for (auto& p : plans) max_steps = p.steps > max_steps ? p.steps : max_steps;
  std::map<Key, long> want_calls;
  long want_rounds = 0;
  for (int r = 0; r < max_steps; r++) {
    std::set<Key> present;
    for (size_t m = 0; m < K; m++)
      if (plans[m].steps > r) present.insert(key_of(m, r));
    want_rounds++;
    if (r == fail_round) {
      want_calls[*present.begin()]++;  // the first group throws, the others of this rendezvous are not served
      if (!resume) break;
    } else {
      for (auto& k : present) want_calls[k]++;
    }
  }
  long want_inv = 0;
  for (auto& kv : want_calls) want_inv += kv.second;
  CHECK((long)gate.rounds() == want_rounds, "K=%zu seed=%llu rounds %zu want %ld", K, (unsigned long long)seed, gate.rounds(), want_rounds);
  CHECK(invocations == want_inv, "K=%zu seed=%llu invocations %ld want %ld", K, (unsigned long long)seed, invocations, want_inv);
  CHECK(calls == want_calls, "K=%zu seed=%llu per-group invocation counts differ", K, (unsigned long long)seed);
  CHECK(gate.inside() == 0, "K=%zu members still inside: %zu", K, gate.inside());
  for (size_t m = 0; m < K; m++) {
    CHECK(wrong[m] == 0, "K=%zu member %zu got %d answers of another payload", K, m, wrong[m]);
    const bool in_failed_round = fail_round >= 0 && plans[m].steps > fail_round;
    CHECK(saw_fail[m] == (in_failed_round ? 1 : 0), "K=%zu member %zu (steps %d) saw the leader's failure %d times", K, m, plans[m].steps, saw_fail[m]);
    const int want_done = in_failed_round && !resume ? (int)fail_round : plans[m].steps;
    CHECK(done_steps[m] == want_done, "K=%zu member %zu finished %d steps, want %d", K, m, done_steps[m], want_done);
  }
}
}  // namespace

int main() {
  const size_t Ks[] = {1, 2, 7, 64};
  const int S = 6;
  long scenarios = 0;
  for (size_t K : Ks) {
    // randomised step counts and ways of leaving
    for (uint64_t seed = 0; seed < (K >= 64 ? 6u : 24u); seed++) {
      std::vector<Plan> plans(K);
      for (size_t m = 0; m < K; m++) {
        uint64_t h = mix(seed * 7919 + m + K * 104729);
        plans[m] = Plan{(int)(h % (S + 1)), ((h >> 8) & 1) != 0};
      }
      run(plans, seed, -1, false), scenarios++;
      run(plans, seed, (long)(seed % S), false), scenarios++;
      run(plans, seed, (long)(seed % S), true), scenarios++;
    }
    // one member leaves at every step position, by return and by exception, while the others go the whole way; the stub throws at every position
    for (int pos = 0; pos <= S; pos++)
      for (int thr = 0; thr < 2; thr++) {
        std::vector<Plan> plans(K, Plan{S, false});
        plans[K / 2] = Plan{pos, thr != 0};
        run(plans, 100 + pos, -1, false), scenarios++;
        if (pos < S) {
          run(plans, 200 + pos, pos, false), scenarios++;
          run(plans, 300 + pos, pos, true), scenarios++;
        }
      }
  }
  // misuse is an error, not a hang: posting after leaving
  {
    Gate g(1, [](const Key&, const std::vector<size_t>&, const std::vector<const uint64_t*>&, std::vector<uint64_t>&) {});
    g.leave(0);
    g.leave(0);
    bool threw = false;
    try { (void)g.post(0, Key{0, 1}, 1); } catch (const std::logic_error&) { threw = true; }
    CHECK(threw, "post after leave did not throw");
    // a serving function that returns too few answers fails the round
    Gate h(1, [](const Key&, const std::vector<size_t>&, const std::vector<const uint64_t*>&, std::vector<uint64_t>&) {});
    threw = false;
    try { (void)h.post(0, Key{0, 1}, 1); } catch (const std::logic_error&) { threw = true; }
    CHECK(threw, "a short answer vector did not throw");
    h.leave(0);
  }
  printf("gate_check: %ld scenarios, %d failures\n", scenarios, g_fail);
  return g_fail ? 1 : 0;
}
