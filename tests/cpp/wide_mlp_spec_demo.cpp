// wide_mlp_spec_demo.cpp — the HIP-free side of rl_mlp_create_wide on the CPU: wide_mlp_shape and rl_rollout's answer to
// a wide module (relearn_amd/csrc/handle_spec.hpp), one line per case on stdout:
//   <name> <code> <in> <out> <P> <general> <wide> <has_bias> | <message>
// tests/test_wide_mlp_spec_cpp.py reads it.
//   g++ -std=c++17 -Wall -Wextra -Werror -I <repo> tests/cpp/wide_mlp_spec_demo.cpp -o demo && ./demo
#include <iostream>
#include <vector>

#include "relearn_amd/csrc/handle_spec.hpp"

static void shape_case(const char *name, uint32_t in_dim, std::vector<uint32_t> hidden, uint32_t out_dim, bool bias,
                       int32_t act = RL_ACT_RELU) {
  try {
    const ModuleShape m = wide_mlp_shape(in_dim, hidden.data(), (uint32_t)hidden.size(), out_dim, act, RL_ACT_IDENTITY, bias);
    std::cout << name << " 0 " << m.in_dim << " " << m.out_dim << " " << m.P << " " << m.general << " " << m.wide << " "
              << m.has_bias << " |\n";
  } catch (const RlError &e) {
    std::cout << name << " " << e.code << " 0 0 0 0 0 0 | " << e.what() << "\n";
  }
}

static void rollout_case(const char *name, int env_kind, uint32_t D, const ModuleShape &m) {
  try {
    const int path = (int)rollout_path(env_kind, D, 2, 0, m);
    std::cout << name << " 0 " << path << " " << (int)ROLL_GENERAL << " 0 0 0 0 |\n";
  } catch (const RlError &e) {
    std::cout << name << " " << e.code << " 0 0 0 0 0 0 | " << e.what() << "\n";
  }
}

int main() {
  shape_case("policy_24", 24, {128}, 2, true);
  shape_case("critic_23_two_layers", 23, {33, 64}, 1, true, RL_ACT_TANH);
  shape_case("nobias_9_no_hidden", 9, {}, 2, false);
  shape_case("fused_5", 5, {128}, 2, true);
  shape_case("general_8", 8, {16}, 3, true);
  shape_case("in_25", 25, {16}, 2, true);
  shape_case("in_0", 0, {16}, 2, true);
  shape_case("out_3_at_24", 24, {16}, 3, true);
  shape_case("out_0_at_24", 24, {16}, 0, true);
  shape_case("out_9_at_24", 24, {16}, 9, true);
  shape_case("width_257_at_9", 9, {257}, 2, true);
  shape_case("four_layers_at_9", 9, {8, 8, 8, 8}, 2, true);
  shape_case("activation_4_at_9", 9, {8}, 2, true, 4);
  const uint32_t h16[1] = {16};
  const ModuleShape wide24 = wide_mlp_shape(24, h16, 1, 2, RL_ACT_RELU, RL_ACT_IDENTITY, true);
  const ModuleShape narrow = wide_mlp_shape(8, h16, 1, 2, RL_ACT_RELU, RL_ACT_IDENTITY, true);
  rollout_case("wide_on_partition", RL_ENV_PARTITION, 24, wide24);
  rollout_case("wide_on_partition_23", RL_ENV_PARTITION, 23, wide24);
  rollout_case("narrow_on_partition", RL_ENV_PARTITION, 24, narrow);
  rollout_case("wide_on_meta_mdp", RL_ENV_META_MDP, 24, wide24);
  return 0;
}
