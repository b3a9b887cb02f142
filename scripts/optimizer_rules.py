"""80 critic steps at 8,192 x 128 with each first-order rule (profiling target: the per-launch time of the reduce + step
kernel per rule, one instantiation of k_reduce_opt<RULE, 16, false> each).
usage: rocprofv3 --kernel-trace --stats ... -- python3 scripts/optimizer_rules.py [lanes] [steps]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra
n, T, steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8192, 128, int(sys.argv[2]) if len(sys.argv) > 2 else 80
eng = ra.Engine(0)
env = ra.CartPoleEnv(eng, n)
pol = ra.Mlp(eng, 5, 128, 2); pol.init(2)
cri = ra.Mlp(eng, 5, 128, 1); cri.init(3)
c0 = cri.get_params()
traj = ra.Trajectory(eng, n, T, 5)
ra.rollout(env, pol, traj); ra.gae(traj, cri, 0.99, 0.95)
RULES = [("adam", ra.OPTIMIZER_ADAM, {}), ("adamw", ra.OPTIMIZER_ADAMW, dict(weight_decay=1e-2)),
         ("sgd momentum (1 state word)", ra.OPTIMIZER_SGD, dict(learning_rate=1e-4, momentum=0.9)),
         ("sgd plain (no state)", ra.OPTIMIZER_SGD, dict(learning_rate=1e-4)),
         ("rmsprop centered + momentum (3 state words)", ra.OPTIMIZER_RMSPROP, dict(learning_rate=1e-3, momentum=0.9, centered=1)),
         ("rmsprop default (1 state word)", ra.OPTIMIZER_RMSPROP, dict(learning_rate=1e-3))]
for name, kind, fields in RULES:
    cfg = ra.optimizer_config_default(kind)
    for k, v in fields.items(): setattr(cfg, k, v)
    cri.set_params(c0)
    opt = ra.Optimizer(cri, cfg)
    ra.critic_update(cri, opt, traj, 3)
    eng.sync(); eng.timer_begin()
    st = ra.critic_update(cri, opt, traj, steps)
    ms = eng.timer_end()
    print("%-46s critic step (gradient + reduce + step): %.2f us (loss %.3f -> %.3f)" % (name, 1e3 * ms / steps, st.loss_first, st.loss_last))
    opt.close()
