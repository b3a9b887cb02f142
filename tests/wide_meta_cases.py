"""The cases of the wide meta-bandit lanes and recurrent chains (rl_env_create_meta_bandit_wide, rl_rnn_chain_create_wide:
5..12 arms, k + 4 = 9..16 observation features, up to 12 outputs) that the CPU test (tests/test_seq_wide_ref.py: the
conditions the tables must meet) and the GPU test (tests/test_gpu_wide_meta.py: the device against the references)
share.  Test infrastructure, not a test.  The references are the existing ones, general in k, D and A:
tests/meta_lanes_ref.py, tests/seq_multi_ref.py, tests/bandit_agents_ref.py, tests/thompson_ref.py.

Why these arm counts: k = 5 has D = 9, the first feature count past eight, with the head still in its class of eight
output registers; 8 (D = 12) is the last of that class; 9 (D = 13) the first of class 12, whose third pass of four rows
holds one live row; 10 (D = 14) is the experiment's default; 12 (D = 16) is the limit, every row of every pass live."""
import meta_lanes_ref as M
import seq_multi_ref as R

# host-written trajectories: T = 5, n in {1, 70}; H in {7, 33}, mlp_hidden in {0, 6}, both cells, one two-layer chain, one
# without recurrent bias vectors
NETS = [
    R.Net("gru", 9, 33, 1, 6, False, 5),    # k = 5; no recurrent bias vectors
    R.Net("lstm", 12, 7, 1, 0, True, 8),    # k = 8: the last of class 8, at twelve inputs
    R.Net("gru", 13, 7, 1, 0, True, 9),     # k = 9: one live row in the third pass
    R.Net("gru", 14, 33, 1, 6, True, 10),   # k = 10
    R.Net("lstm", 16, 33, 2, 6, True, 12),  # k = 12: two layers, every row of three passes
    R.Net("lstm", 16, 7, 1, 0, True, 12),
]
CRITICS = [R.Net("gru", 14, 7, 1, 0, True, 1), R.Net("lstm", 16, 33, 1, 6, True, 2)]  # wide inputs, output class 2

# closed-loop rollouts (tests/seq_multi_ref.py: meta_rollout): T = 13 at 3 episodes per trial — trials end at steps 5 and
# 10 and the horizon cuts the third; seed: the module's init seed, seed_env = seed + 1, seed_actor = seed + 2, chosen so
# that every sampled action is decided by more than R.MIN_MARGIN (tests/test_seq_wide_ref.py checks it and prints the margins)
META_CASES = [
    R.MetaCase(R.Net("gru", 9, 7, 1, 0, True, 5), 70, 13, 3, M.UNIFORM_BERNOULLI, 0, 501),
    R.MetaCase(R.Net("lstm", 9, 7, 1, 6, True, 5), 1, 13, 3, M.ONE_HOT, 0, 511),       # one lane
    R.MetaCase(R.Net("lstm", 13, 7, 2, 6, True, 9), 70, 13, 3, M.ONE_HOT, 25, 523),    # two layers; lanes 25..94
    R.MetaCase(R.Net("gru", 14, 33, 1, 0, True, 10), 70, 13, 3, M.UNIFORM_BERNOULLI, 0, 531),
    R.MetaCase(R.Net("gru", 16, 7, 1, 6, False, 12), 70, 13, 3, M.UNIFORM_BERNOULLI, 0, 542),
    R.MetaCase(R.Net("lstm", 16, 33, 1, 0, True, 12), 70, 13, 3, M.ROUND_ROBIN, 0, 554),
]

# the clipped PPO gradient off ratio 1: (net, SGD rate); the rate is chosen on the CPU (the f64 oracle's step from the
# same start, tests/test_seq_wide_ref.py) so that the first step clips at least a twentieth of the samples at clip
# distance 0.2, leaves as many unclipped, and leaves no ratio within 3e-4 of a bound
# (with nine and twelve near-uniform actions a logit moves a probability less than with three: the rates are larger than
# tests/test_gpu_seq_multi_action.py's)
PPO_CASES = [(R.Net("gru", 13, 12, 1, 6, True, 9), 16.0), (R.Net("lstm", 16, 12, 1, 0, True, 12), 48.0)]
PPO_N, PPO_T, PPO_INIT_SEED, PPO_HISTORY_SEED = 70, 5, 51, 8


def pack_lane_byte(done, some, action):
    """the byte a meta lane keeps beside its words (env_lanes.hpp, MetaOps::store): bit 0 inner episode done, bit 1
    prev_step_obs is Some, bits 2-5 its action"""
    return (done & 1) | ((some & 1) << 1) | (action << 2)


def unpack_lane_byte(b):
    return b & 1, (b >> 1) & 1, (b >> 2) & 15
