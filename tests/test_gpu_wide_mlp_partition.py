"""rl_rollout of a feed-forward ra.MlpWide policy on PartitionGame lanes (23 features under a latent limit, 24 under a
visible one): the env side against the Python lanes of tests/partition_ref.py driven by the device's own actions, bit for
bit; the logits rl_mlp_forward gives for the collected observations against numpy f64 within the f32 chain's bound
(logit_bound, tests/test_gpu_wide_mlp.py) and the recorded actions against the oracle's inverse-CDF draw from those logits with the
lane's actor word; then one rl_actor_critic_update on what was collected.  Fails on a library without rl_mlp_create_wide."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import partition_cases as W
import partition_ref as P
import relearn_amd as ra
from test_gpu_wide_mlp import forward64, logit_bound

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("limit", [W.VISIBLE3, W.LATENT3], ids=W.limit_id)
def test_rollout_and_update_on_partition_lanes(engine, limit):
    n, T, D = 64, W.HORIZON, P.obs_dim(limit)
    env = ra.PartitionEnv(engine, n, max_steps=limit.max_steps, limit=limit.kind, seed_env=3, seed_actor=4)
    assert (env.D, env.A) == (D, 2)
    pol, cri = ra.MlpWide(engine, D, [16], 2), ra.MlpWide(engine, D, [16], 1)
    pol.init(31), cri.init(32)
    traj = ra.TrajectoryWide24(engine, n, T, D)
    ra.rollout(env, pol, traj)
    got = traj.read_all()
    ref = P.PartitionLanes(n, limit, seed_env=3)
    assert np.array_equal(got["obs"][:, 0], ref.observe())
    for t in range(T):
        reward, flag, obs, term = ref.step(got["action"][t])
        assert np.array_equal(got["reward"][t], reward) and np.array_equal(got["flag"][t], flag), t
        assert np.array_equal(got["obs"][:, t + 1], obs), t
        cut = flag == P.INTERRUPT
        assert np.array_equal(got["term_obs"][:, t][:, cut], term[:, cut]), t
    assert sorted(np.unique(got["action"])) == [0, 1] and (got["flag"] == P.INTERRUPT).sum() == 2 * n
    x = got["obs"][:, :T].reshape(D, T * n).T
    z, p = pol.forward(x), pol.get_params()
    c = (D, [16], "Relu", True)
    z64 = forward64(torch.tensor(p.astype(np.float64)), [D, 16, 2], "Relu", True, torch.tensor(x.astype(np.float64))).numpy()
    assert np.abs(z - z64).max() <= logit_bound(c, p, x) and np.ptp(z) > 0
    # PolicyActor::act as tests/test_gpu_multi_action.py replays it: word t of the lane's actor stream against the oracle's
    # log-softmax and inverse-CDF draw on the device's logits
    for t in (0, T - 1):
        for i in range(n):
            u = np.float32(engine.stream_words(4, i, t, 1)[0] >> 8) * np.float32(1.0 / (1 << 24))
            lp = np.zeros(2, dtype=np.float32)
            O.lib().oracle_log_softmax_f32(O.f32p(np.ascontiguousarray(z[t * n + i])), 2, O.f32p(lp), 0)
            assert got["action"][t][i] == O.lib().oracle_categorical_sample_u(O.f32p(lp), 2, C.c_float(u), 0), (t, i)
    p0 = pol.get_params()
    ra.gae(traj, cri, 0.999, 0.95)
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 3
    st, cst = ra.actor_critic_update(pol, cri, ra.Adam(cri), traj, None, ccfg)
    assert st.status == ra.OPT_OK and st.loss_final < st.loss_initial and cst.loss_last < cst.loss_first
    assert not np.array_equal(pol.get_params(), p0) and np.all(np.isfinite(pol.get_params()))
