// env_shape.hpp — an env's lane family and feature count as constants: the table of handle_spec.hpp (EnvLanes,
// ENV_LANE_FEATURES) looked up through dispatch.hpp.  env_dispatch (env_lanes.hpp) adds the ops struct.  Plain C++17
// without a HIP include: tests/cpp/dispatch_demo.cpp.
#pragma once

#include "dispatch.hpp"
#include "handle_spec.hpp"

// go(Int<family>{}): the family half alone (k_env_reset is built per ops struct)
template <class Go>
void with_env_lanes(int kind, uint32_t meta_mdp_states, Go &&go) {
  if (!with_range<0, ENV_LANES_COUNT - 1>(env_lanes_of(kind, meta_mdp_states), go))
    throw RlError(RL_ERR_UNSUPPORTED, "env kernels: a lane family without a table entry");
}
// go(Int<family>{}, Int<D>{}) for a feature count inside the family's range, the family's refusal for any other
template <class Go>
void with_env_shape(int kind, uint32_t meta_mdp_states, uint32_t D, Go &&go) {
  with_env_lanes(kind, meta_mdp_states, [&](auto lanes) {
    constexpr LaneFeatures f = ENV_LANE_FEATURES[decltype(lanes)::value];
    if (!with_range<f.lo, f.hi>(D, [&](auto d) { go(lanes, d); })) throw RlError(RL_ERR_UNSUPPORTED, f.refusal);
  });
}
