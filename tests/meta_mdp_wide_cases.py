"""Case tables of the meta-MDP lanes behind rl_env_create_meta_mdp_wide (test infrastructure, not a test): the lanes of
tests/meta_mdp_ref.py — imported unchanged; they take any size — at the shapes the wider entry point adds, with the reason
for each shape.  tests/test_meta_mdp_wide_cases.py pins the tables' own conditions on the CPU, the margin of every sampled
action among them; the GPU tests run the device against the references computed here, once per process.

  (10, 5)  DirichletRandomMdps::default, the RL^2 paper's tabular-MDP task: 19 features; the shape whose rollout is one
           launch (META_MDP_WIDE_FUSED_SHAPES)
  (9, 2)   the smallest shape of the 16-float row: nine states, 15 features — narrower than rows of eight floats reach
  (10, 6)  20 features, the most the entry point takes; the launch sequence per step
  (8, 8)   the OLD row class behind the NEW entry point: rows of eight floats under 20 features, which
           rl_env_create_meta_mdp refuses (it ends at 16)"""
import meta_mdp_ref as M
import seq_multi_ref as R

dist = M.dist
N_LANES, OFFSET, TRIALS = M.N_LANES, M.OFFSET, M.TRIALS  # 70 lanes, the 45 lanes at offset 25, three trials and a step

SHAPES = {
    (10, 5): "the default and the fused shape",
    (9, 2): "the smallest shape of the 16-float row",
    (10, 6): "20 features, the most",
    (8, 8): "the old row class behind the new entry point",
}

# driven steps: short trials, so that three trials and a step stay a few seconds of Python; every Gamma path
DRIVEN = [
    M.Driven(dist(10, 5, 2, 3), 61, SHAPES[(10, 5)]),
    M.Driven(dist(10, 5, 1, 2, alpha=0.5, reward_stddev=0.5), 62, "10 x 5 on the Gamma path below 1"),
    M.Driven(dist(9, 2, 2, 2, alpha=2.5), 63, SHAPES[(9, 2)] + "; Marsaglia-Tsang"),
    M.Driven(dist(10, 6, 2, 2), 64, SHAPES[(10, 6)]),
    M.Driven(dist(8, 8, 2, 2, reward_stddev=0.0), 65, SHAPES[(8, 8)] + "; no per-step normal draw"),
]
driven_id, driven_steps, driven_reference = M.driven_id, M.driven_steps, M.driven_reference

# closed loop: hidden width 8, T = 7 against trials of 5 steps (E = 2, L = 2), so that a trial runs across the two
# collections.  (10, 5): both cells, both tails, 70 lanes, and the 45 lanes at offset 25; (9, 2) and (10, 6): per step.
# seed: the module's init seed, seed_env = seed + 1, seed_actor = seed + 2 — chosen on the CPU so that every sampled
# action is decided by more than MIN_MARGIN (tests/test_meta_mdp_wide_cases.py prints the margins).
CLOSED = [
    M.Closed(R.Net("gru", 19, 8, 1, 0, True, 5), dist(10, 5, 2, 2), 70, 7, 0, 601),
    M.Closed(R.Net("gru", 19, 8, 1, 6, True, 5), dist(10, 5, 2, 2), 70, 7, 0, 611),
    M.Closed(R.Net("lstm", 19, 8, 1, 0, True, 5), dist(10, 5, 2, 2), 45, 7, 25, 622),
    M.Closed(R.Net("lstm", 19, 8, 1, 6, False, 5), dist(10, 5, 2, 2), 70, 7, 0, 631),
    M.Closed(R.Net("gru", 15, 8, 1, 0, True, 2), dist(9, 2, 2, 2), 70, 7, 0, 641),
    M.Closed(R.Net("lstm", 20, 8, 1, 6, True, 6), dist(10, 6, 2, 2), 70, 7, 0, 651),
]
FUSED = [(10, 5)]  # handle_spec.hpp's META_MDP_WIDE_FUSED_SHAPES
closed_id, closed_reference, closed_params, PERIODS = M.closed_id, M.closed_reference, M.closed_params, M.PERIODS
