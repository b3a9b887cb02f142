// envs.hpp — scalar host-side mirrors of the reference's environment interface (src/envs/mod.rs:76-127,
// 257-269): `initial_state(rng)`, `observe(state, rng)`, `step(state, action, rng) -> (Successor<State>, reward)`.
// Used by the CPU-only plumbing configuration (Chain + tabular Q) and as the scalar view of what the lanes do.
#pragma once
#include <cmath>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../../include/rl_normal.h"
#include "prng.hpp"

namespace relearn {

// Successor<T> (src/envs/mod.rs:257-269)
enum class SuccessorKind : uint8_t { Continue = 0, Terminate = 1, Interrupt = 2 };

template <typename T>
struct Successor {
  SuccessorKind kind = SuccessorKind::Terminate;
  std::optional<T> state;  // present for Continue and Interrupt

  static Successor Continue(T s) { return {SuccessorKind::Continue, std::move(s)}; }
  static Successor Terminate() { return {SuccessorKind::Terminate, std::nullopt}; }
  static Successor Interrupt(T s) { return {SuccessorKind::Interrupt, std::move(s)}; }
  bool episode_done() const { return kind != SuccessorKind::Continue; }
  // then_interrupt_if (src/envs/mod.rs:348-362)
  template <typename F>
  Successor then_interrupt_if(F &&f) && {
    if (kind == SuccessorKind::Continue && f(*state)) kind = SuccessorKind::Interrupt;
    return std::move(*this);
  }
  template <typename U, typename F>
  Successor<U> map(F &&f) && {
    if (kind == SuccessorKind::Terminate) return Successor<U>::Terminate();
    Successor<U> out;
    out.kind = kind;
    out.state = f(std::move(*state));
    return out;
  }
};

// Chain (src/envs/chain.rs:20-106): n states in a line, 2 actions, 0.2 slip probability
struct Chain {
  using State = uint64_t;
  using Observation = uint64_t;
  using Action = uint8_t;  // Move::Left = 0, Move::Right = 1
  uint64_t size = 5;
  double discount_factor = 0.95;

  uint64_t num_observations() const { return size; }
  uint64_t num_actions() const { return 2; }
  State initial_state(Prng &) const { return 0; }
  Observation observe(const State &s, Prng &) const { return s; }
  std::pair<Successor<State>, double> step(State s, Action a, Prng &rng) const {
    if (rng.gen_f32() < 0.2f) a = a ? 0 : 1;  // Move::invert
    if (a == 0) return {Successor<State>::Continue(0), 2.0};
    if (s == size - 1) return {Successor<State>::Continue(s), 10.0};
    return {Successor<State>::Continue(s + 1), 0.0};
  }
};

// MemoryGame (src/envs/memory.rs:24-115): start in one of `num_actions` states at random, walk through `history_len`
// further states whatever the action, then answer: +1 iff the action equals the initial state, else -1 (terminal)
struct MemoryGame {
  using State = std::pair<uint64_t, uint64_t>;  // (current_state, initial_state)
  using Observation = uint64_t;
  using Action = uint64_t;
  uint64_t num_actions_ = 2, history_len = 1;  // MemoryGame::default
  double discount_factor = 1.0;

  MemoryGame() = default;
  MemoryGame(uint64_t num_actions, uint64_t history) : num_actions_(num_actions), history_len(history) {}
  uint64_t num_observations() const { return num_actions_ + history_len; }
  uint64_t num_actions() const { return num_actions_; }
  State initial_state(Prng &rng) const {
    const uint64_t s = rng.gen_range(0, num_actions_);
    return {s, s};
  }
  Observation observe(const State &s, Prng &) const { return s.first; }
  std::pair<Successor<State>, double> step(State s, Action a, Prng &) const {
    if (s.first == num_actions_ + history_len - 1) return {Successor<State>::Terminate(), a == s.second ? 1.0 : -1.0};
    const uint64_t next = s.first < num_actions_ ? num_actions_ : s.first + 1;
    return {Successor<State>::Continue({next, s.second}), 0.0};
  }
};

// TabularMdp<_, Normal<f64>> (src/envs/mdps.rs:12-85) as the lanes state it (include/relearn_hip.h,
// rl_env_create_tabular_mdp): starts in state 0; a step draws one u64 for the successor — always — and counts the entries
// of the row's f32 running sum at or below the low word's unit float, then draws the reward's polar normal
// (include/rl_normal.h) unless the row's stddev is 0.  No terminal states.
struct TabularMdp {
  using State = uint64_t;
  using Observation = uint64_t;
  using Action = uint64_t;
  uint64_t num_states = 0, num_actions_ = 0;
  std::vector<float> transitions;            // [S][A][S]
  std::vector<float> cumulative;             // [S][A][S], formed by the constructor
  std::vector<double> reward_mean, reward_stddev;  // [S][A]
  double discount_factor = 1.0;

  TabularMdp() = default;
  // `stddev` empty: 1.0 everywhere (DirichletRandomMdps, mdps.rs:163)
  TabularMdp(uint64_t S, uint64_t A, std::vector<float> tr, std::vector<double> mean, std::vector<double> stddev = {},
             double discount = 1.0)
      : num_states(S), num_actions_(A), transitions(std::move(tr)), reward_mean(std::move(mean)),
        reward_stddev(std::move(stddev)), discount_factor(discount) {
    if (S == 0 || A == 0 || transitions.size() != S * A * S || reward_mean.size() != S * A)
      throw std::invalid_argument("TabularMdp: tables of [S][A][S] and [S][A]");
    if (reward_stddev.empty()) reward_stddev.assign(S * A, 1.0);
    if (reward_stddev.size() != S * A) throw std::invalid_argument("TabularMdp: reward_stddev of [S][A]");
    cumulative.resize(transitions.size());
    // the running sums, from the row's last possible successor on exactly 1: the one statement the lanes share
    for (uint64_t row = 0; row < S * A; ++row)
      rl_mdp_row_cumulative(transitions.data() + row * S, (uint32_t)S, (uint32_t)S, cumulative.data() + row * S);
  }
  uint64_t num_observations() const { return num_states; }
  uint64_t num_actions() const { return num_actions_; }
  State initial_state(Prng &) const { return 0; }
  Observation observe(const State &s, Prng &) const { return s; }
  // the polar normal from a sequential generator: two u64 per attempt, at most RL_NORMAL_MAX_ATTEMPTS attempts
  static double normal(Prng &rng) {
    double z = 0.0;
    for (int attempt = 0; attempt < RL_NORMAL_MAX_ATTEMPTS; ++attempt) {
      const uint64_t w1 = rng.next_u64(), w2 = rng.next_u64();
      if (rl_normal_attempt(w1, w2, &z)) break;
    }
    return z;
  }
  std::pair<Successor<State>, double> step(State s, Action a, Prng &rng) const {
    const uint64_t row = s * num_actions_ + a;
    const float u = rl_u32_to_unit_f32((uint32_t)rng.next_u64());
    State next = 0;
    for (uint64_t j = 0; j + 1 < num_states; ++j) next += cumulative[row * num_states + j] <= u ? 1 : 0;
    double reward = reward_mean[row];
    if (reward_stddev[row] != 0.0) reward = reward_mean[row] + reward_stddev[row] * normal(rng);
    return {Successor<State>::Continue(next), reward};
  }
};

// DirichletRandomMdps (src/envs/mdps.rs:87-171): the distribution over MDPs of the second task of the RL^2 paper.
// sample_environment consumes ONE stream — ChaCha8Rng::seed_from_u64(seed), set_stream(stream) — sequentially, row-major
// over (s, a): the S Gamma(alpha, 1) draws of the row's Dirichlet sample (include/rl_normal.h), normalised in f64 and each
// cast to f32, then the row's reward mean.  rl_random_mdps_sample is this function.
struct DirichletRandomMdps {
  uint64_t num_states = 10, num_actions = 5;
  double transition_prior_dirichlet_alpha = 1.0, reward_prior_mean = 1.0, reward_prior_stddev = 1.0;
  double discount_factor = 1.0;  // (assumes a step limit on the episodes)

  // throws std::invalid_argument naming the field
  void validate() const {
    if (num_states < 1 || num_states > 64 || num_actions < 1 || num_actions > 64)
      throw std::invalid_argument("DirichletRandomMdps: num_states and num_actions in 1..64");
    if (!std::isfinite(transition_prior_dirichlet_alpha) || !(transition_prior_dirichlet_alpha > 0.0))
      throw std::invalid_argument("DirichletRandomMdps: transition_prior_dirichlet_alpha must be positive and finite");
    if (!std::isfinite(reward_prior_mean))
      throw std::invalid_argument("DirichletRandomMdps: reward_prior_mean must be finite");
    if (!std::isfinite(reward_prior_stddev) || reward_prior_stddev < 0.0)
      throw std::invalid_argument("DirichletRandomMdps: reward_prior_stddev must be non-negative and finite");
    if (!std::isfinite(discount_factor)) throw std::invalid_argument("DirichletRandomMdps: discount_factor must be finite");
  }
  // transitions [S][A][S], reward_mean [S][A]
  void sample_tables(uint64_t seed, uint64_t stream, float *transitions, double *reward_mean) const {
    uint32_t key[8];
    rl_seed_from_u64(seed, key);
    uint64_t pos = 0;
    sample_tables_at(key, stream, &pos, transitions, reward_mean);
  }
  // the same draws from a sequential generator where it stands, which moves behind them: a meta env's trial start
  void sample_tables_from(Prng &rng, float *transitions, double *reward_mean) const {
    uint64_t pos = rng.word_pos();
    sample_tables_at(rng.key(), rng.stream(), &pos, transitions, reward_mean);
    rng.set_word_pos(pos);
  }
  // ... from word `*pos` (even) of the stream (key, stream); `*pos` moves behind the last word read
  void sample_tables_at(const uint32_t key[8], uint64_t stream, uint64_t *pos_io, float *transitions,
                        double *reward_mean) const {
    validate();
    uint64_t pos = *pos_io;
    const uint64_t S = num_states, A = num_actions;
    double g[64];
    for (uint64_t row = 0; row < S * A; ++row) {
      double sum = 0.0;  // Dirichlet::sample: S Gamma(alpha, 1) draws, normalised
      for (uint64_t j = 0; j < S; ++j) {
        g[j] = rl_gamma_sample(transition_prior_dirichlet_alpha, key, stream, &pos);
        sum = sum + g[j];
      }
      rl_dirichlet_row_normalise(g, sum, (uint32_t)S, (uint32_t)S, transitions + row * S);
      // Normal::new(reward_prior_mean, reward_prior_stddev).sample
      reward_mean[row] = reward_prior_mean + reward_prior_stddev * rl_normal_sample(key, stream, &pos);
    }
    *pos_io = pos;
  }
  TabularMdp sample_environment(uint64_t seed, uint64_t stream = 0) const {
    validate();
    std::vector<float> tr(num_states * num_actions * num_states);
    std::vector<double> mean(num_states * num_actions);
    sample_tables(seed, stream, tr.data(), mean.data());
    return TabularMdp(num_states, num_actions, std::move(tr), std::move(mean), {}, discount_factor);
  }
};

// PartitionGame (src/envs/partition.rs:11-130): a supervisor classifies elements of ten booleans by one axis, drawn at the
// episode's start; the action classifies the current element (ClassifyLeft 0, ClassifyRight 1) and earns +1 when it is the
// supervisor's label, else -1; the next observation carries the element just judged and its label.  Never terminates.
// Draws, as the lanes of rl_env_create_partition state them (include/relearn_hip.h): gen_range(0..10) for the axis, then
// ten gen::<bool>() — one next_u32 each, the sign bit is the value — per element, in index order.
struct PartitionGame {
  static constexpr uint64_t NUM_FEATURES = 10;
  using Action = uint64_t;
  using Observation = std::vector<float>;
  struct State {
    uint64_t axis = 0;      // Supervisor::AxisAligned(axis)
    uint32_t element = 0;   // bit j = element[j]
    bool feedback = false;  // Some((prev_element, label))
    uint32_t prev_element = 0;
    uint32_t label = 0;     // Classification: Left 0, Right 1
  };
  double discount_factor = 0.999;

  uint64_t num_observation_features() const { return 2 * NUM_FEATURES + 3; }
  uint64_t num_actions() const { return 2; }
  static uint32_t gen_element(Prng &rng) {
    uint32_t e = 0;
    for (uint64_t j = 0; j < NUM_FEATURES; ++j) e |= (rng.next_u32() >> 31) << j;  // (x as i32) < 0
    return e;
  }
  State initial_state(Prng &rng) const {
    State s;
    s.axis = rng.gen_range(0, NUM_FEATURES);
    s.element = gen_element(rng);
    return s;
  }
  // [element, 10] [feedback is None] [previous element, 10] [one-hot label: Left, Right]
  Observation observe(const State &s, Prng &) const {
    Observation f(num_observation_features(), 0.0f);
    for (uint64_t j = 0; j < NUM_FEATURES; ++j) f[j] = (s.element >> j) & 1u ? 1.0f : 0.0f;
    if (s.feedback) {
      for (uint64_t j = 0; j < NUM_FEATURES; ++j) f[NUM_FEATURES + 1 + j] = (s.prev_element >> j) & 1u ? 1.0f : 0.0f;
      f[2 * NUM_FEATURES + 1 + s.label] = 1.0f;
    } else {
      f[NUM_FEATURES] = 1.0f;
    }
    return f;
  }
  std::pair<Successor<State>, double> step(State s, Action a, Prng &rng) const {
    const uint32_t label = (s.element >> s.axis) & 1u;
    const double reward = a == label ? 1.0 : -1.0;
    s.feedback = true;
    s.prev_element = s.element;
    s.label = label;
    s.element = gen_element(rng);
    return {Successor<State>::Continue(std::move(s)), reward};
  }
};

// Wrapped<E, LatentStepLimit> (src/envs/wrappers/step_limit.rs:13-89): the limit is not observable
template <typename E>
struct WithLatentStepLimit {
  struct State {
    typename E::State inner;
    uint64_t steps_remaining;
  };
  using Observation = typename E::Observation;
  using Action = typename E::Action;
  E inner;
  uint64_t max_steps_per_episode = 100;

  uint64_t num_observations() const { return inner.num_observations(); }
  uint64_t num_actions() const { return inner.num_actions(); }
  State initial_state(Prng &rng) const { return {inner.initial_state(rng), max_steps_per_episode}; }
  Observation observe(const State &s, Prng &rng) const { return inner.observe(s.inner, rng); }
  std::pair<Successor<State>, double> step(State s, Action a, Prng &rng) const {
    auto [succ, reward] = inner.step(std::move(s.inner), a, rng);
    const uint64_t left = s.steps_remaining - 1;
    auto wrapped = std::move(succ).template map<State>([&](typename E::State in) { return State{std::move(in), left}; });
    return {std::move(wrapped).then_interrupt_if([](const State &n) { return n.steps_remaining == 0; }), reward};
  }
};

// Wrapped<E, VisibleStepLimit> (src/envs/wrappers/step_limit.rs:97-222) over an env whose observation is its feature
// vector: the observation carries `remaining / max` as one more feature (f64 quotient, then `as f32`), which is what the
// lanes write under RL_LIMIT_VISIBLE.  partition-game.rs wraps PartitionGame in VisibleStepLimit::new(1000).
template <typename E>
struct WithVisibleStepLimit {
  using State = typename WithLatentStepLimit<E>::State;
  using Observation = std::vector<float>;
  using Action = typename E::Action;
  E inner;
  uint64_t max_steps_per_episode = 100;

  uint64_t num_observation_features() const { return inner.num_observation_features() + 1; }
  uint64_t num_actions() const { return inner.num_actions(); }
  State initial_state(Prng &rng) const { return {inner.initial_state(rng), max_steps_per_episode}; }
  Observation observe(const State &s, Prng &rng) const {
    Observation f = inner.observe(s.inner, rng);
    f.push_back((float)((double)s.steps_remaining / (double)max_steps_per_episode));
    return f;
  }
  // the latent wrapper's step: the two differ in what they show, not in when they cut
  std::pair<Successor<State>, double> step(State s, Action a, Prng &rng) const {
    return WithLatentStepLimit<E>{inner, max_steps_per_episode}.step(std::move(s), a, rng);
  }
};

// Wrapped<MetaEnv<Wrapped<DirichletRandomMdps, LatentStepLimit>>, TrialEpisodeLimit> (src/envs/meta.rs:128-203, 541-617
// over mdps.rs:87-171 and wrappers/step_limit.rs:13-89), the second task of the RL^2 paper, as the lanes of
// rl_env_create_meta_mdp state it (include/relearn_hip.h): a trial starts with sample_environment from the env generator
// where it stands; an inner episode is max_inner_steps steps of TabularMdp::step and ends in the limit's Interrupt(state);
// the step after it ignores its action, draws nothing and starts the next inner episode; the step that ends the trial's
// last inner episode is an Interrupt.  The scalar env takes any size the sampler takes; the lanes end at 10 x 8 and 20
// features (rl_env_create_meta_mdp_wide).  One generator, seed_from_u64(seed_env) on stream g, gives lane g's trials.
struct MetaRandomMdps {
  using Action = uint64_t;
  using Observation = std::vector<float>;
  struct State {
    TabularMdp mdp;  // the trial's MDP
    uint64_t inner_state = 0, inner_left = 0, episodes_left = 0;
    bool inner_done = false;  // inner_successor is Interrupt(inner_state)
    bool prev_some = false;   // prev_step_obs: Some(InnerStepObs { action, feedback })
    uint64_t prev_action = 0;
    float prev_reward = 0.0f;
  };
  DirichletRandomMdps dist;
  uint64_t max_inner_steps = 10, episodes_per_trial = 10;
  double reward_stddev = 1.0;  // of every sampled MDP's rewards (mdps.rs:163)

  void validate() const {
    dist.validate();
    if (max_inner_steps == 0) throw std::invalid_argument("MetaRandomMdps: max_inner_steps must be positive");
    if (episodes_per_trial == 0) throw std::invalid_argument("MetaRandomMdps: trials must contain at least 1 episode");
    if (!std::isfinite(reward_stddev) || reward_stddev < 0.0)
      throw std::invalid_argument("MetaRandomMdps: reward_stddev must be non-negative and finite");
  }
  uint64_t num_observation_features() const { return dist.num_states + dist.num_actions + 4; }
  uint64_t num_actions() const { return dist.num_actions; }
  uint64_t trial_steps() const { return episodes_per_trial * (max_inner_steps + 1) - 1; }
  // TrialEpisodeLimit / MetaEnv::initial_state: sample_environment, then the inner initial_state (state 0, no draw)
  State initial_state(Prng &rng) const {
    validate();
    const uint64_t S = dist.num_states, A = dist.num_actions;
    std::vector<float> tr(S * A * S);
    std::vector<double> mean(S * A);
    dist.sample_tables_from(rng, tr.data(), mean.data());
    State s;
    s.mdp = TabularMdp(S, A, std::move(tr), std::move(mean), std::vector<double>(S * A, reward_stddev), dist.discount_factor);
    s.inner_left = max_inner_steps;
    s.episodes_left = episodes_per_trial;
    return s;
  }
  // [inner is None] [one-hot(inner state), S] [prev is None] [one-hot(prev action), A] [prev reward] [episode_done]
  Observation observe(const State &s, Prng &) const {
    const uint64_t S = dist.num_states, A = dist.num_actions;
    Observation f(S + A + 4, 0.0f);
    f[1 + s.inner_state] = 1.0f;
    if (s.prev_some) {
      f[2 + S + s.prev_action] = 1.0f;
      f[2 + S + A] = s.prev_reward;
    } else {
      f[1 + S] = 1.0f;
    }
    f[S + A + 3] = s.inner_done ? 1.0f : 0.0f;
    return f;
  }
  // (an action outside 0 .. num_actions - 1 is the caller's error, as on TabularMdp)
  std::pair<Successor<State>, double> step(State s, Action a, Prng &rng) const {
    if (s.inner_done) {  // the action is ignored, nothing is drawn
      s.inner_state = 0;
      s.inner_left = max_inner_steps;
      s.inner_done = false;
      s.prev_some = false;
      s.prev_action = 0;
      s.prev_reward = 0.0f;
      return {Successor<State>::Continue(std::move(s)), 0.0};
    }
    auto [succ, reward] = s.mdp.step(s.inner_state, a, rng);
    s.inner_state = *succ.state;
    s.prev_some = true;
    s.prev_action = a;
    s.prev_reward = (float)reward;
    const double outer = (double)s.prev_reward;
    s.inner_left -= 1;
    if (s.inner_left == 0) {
      s.inner_done = true;
      s.episodes_left -= 1;
      if (s.episodes_left == 0) return {Successor<State>::Interrupt(std::move(s)), outer};
    }
    return {Successor<State>::Continue(std::move(s)), outer};
  }
};

}  // namespace relearn
