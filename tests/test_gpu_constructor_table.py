"""What every env and module constructor refuses (status code and words, and which of two refusals comes first) and what
it decides and allocates for the shapes it accepts, pinned against a recorded table.

The cases are tests/constructor_cases.py; every one is made through the C ABI with raw ctypes (no wrapper class tidies
an argument on the way).  Per case the table holds the status code and rl_last_error's message, or rl_env_dims /
rl_mlp_num_params, with the rise of live device bytes and allocations over the create (rl_debug_device_memory) — both
must be back where they started after the destroy, and a refused create must leave them alone.  The NULL-argument
refusals, which only a caller of the C ABI can provoke, are listed here (null_cases).

    python tests/test_gpu_constructor_table.py --record [--out FILE]

writes the table (run it on the commit whose answers are to be pinned; the file is never edited by hand).
tests/test_handle_spec_cpp.py holds the HIP-free half of the constructors to the same file on the CPU.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import relearn_amd as ra  # noqa: E402
import constructor_cases as CC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "constructor_table.json")
u32, i32, u64 = C.c_uint32, C.c_int32, C.c_uint64


def env_config(kind, limit, max_steps, n_lanes, chain_size=0, mem_actions=0, mem_history=0):
    cfg = ra.EnvConfig()
    cfg.kind, cfg.limit_kind, cfg.max_steps, cfg.n_lanes = kind, limit, max_steps, n_lanes
    cfg.seed_env, cfg.seed_actor, cfg.cartpole = 3, 4, ra.cartpole_params_default()
    cfg.chain_size, cfg.memory_num_actions, cfg.memory_history_len = chain_size, mem_actions, mem_history
    cfg.bandit_values[0], cfg.bandit_values[1] = 0.0, 1.0
    return cfg


def mdp_tables(S, A, table):
    """the tables of an mdp case (constructor_cases.py)"""
    tr = np.full((S * A, S), np.float32(1.0 / S), dtype=np.float32)
    mean = 0.25 * np.arange(S * A, dtype=np.float64)
    sd = None
    if table == 1:
        tr[3, 0] = -0.5
    if table in (2, 6):
        tr[1, 0] = 0.0
    if table in (3, 6):
        mean[2] = np.inf
    if table in (4, 5):
        sd = np.full(S * A, 0.5)
    if table == 4:
        sd[1] = -1.0
    return tr, mean, sd


def initializers(nums):
    """(given kind scale value) groups -> rl_initializer pointers, NULL where not given"""
    keep, ptrs = [], []
    for i in range(0, len(nums), 4):
        given, kind, scale, value = nums[i:i + 4]
        keep.append(ra.Initializer(int(kind), int(scale), float(value)))
        ptrs.append(C.byref(keep[-1]) if given else None)
    return keep, ptrs


def create(eng, ctor, nums, n_lanes=None):
    """one constructor call -> (status code, handle, "env" | "module")"""
    L, h = ra.lib(), C.c_void_p()
    out = C.byref(h)
    if ctor in ("env", "bandit", "meta", "meta_wide", "mdp", "meta_as", "meta_wide_as", "mdp_as"):
        if ctor in ("env", "bandit"):
            cfg = env_config(*nums[:4]) if ctor == "bandit" else env_config(*nums)
        elif ctor.endswith("_as"):  # the config says another kind (and a MemoryGame shape): the constructor names its own
            ctor, (kind, mem_actions, mem_history), nums = ctor[:-3], nums[:3], nums[3:]
            cfg = env_config(kind, *nums[:3], mem_actions=mem_actions, mem_history=mem_history)
        else:
            cfg = env_config(ra.ENV_CARTPOLE, *nums[:3])
        if n_lanes is not None:
            cfg.n_lanes = n_lanes
        if ctor == "env":
            rc = L.rl_env_create(eng.h, C.byref(cfg), out)
        elif ctor == "bandit":
            values = (C.c_double * nums[4])(*[0.5 * a - 1.0 for a in range(nums[4])])
            rc = L.rl_env_create_bandit(eng.h, C.byref(cfg), values, u32(nums[4]), out)
        elif ctor in ("meta", "meta_wide"):
            meta = ra.MetaBanditConfig(nums[3], nums[4], nums[5])
            fn = L.rl_env_create_meta_bandit if ctor == "meta" else L.rl_env_create_meta_bandit_wide
            rc = fn(eng.h, C.byref(cfg), C.byref(meta), out)
        else:
            S, A = nums[3], nums[4]
            mdp = ra.TabularMdpConfig(S, A, float(nums[5]))
            tr, mean, sd = mdp_tables(S, A, nums[6])
            rc = L.rl_env_create_tabular_mdp(eng.h, C.byref(cfg), C.byref(mdp), tr.ctypes.data_as(C.c_void_p),
                                             mean.ctypes.data_as(C.c_void_p),
                                             sd.ctypes.data_as(C.c_void_p) if sd is not None else None, out)
        return rc, h, "env"
    if ctor == "mlp":
        rc = L.rl_mlp_create(eng.h, u32(nums[0]), u32(nums[1]), u32(nums[2]), out)
    elif ctor in ("mlp_layers", "mlp_config"):
        k = 4 if ctor == "mlp_layers" else 5
        widths = nums[k + 1:]
        assert len(widths) == nums[k]
        sizes = (u32 * max(len(widths), 1))(*widths)
        head = [eng.h, u32(nums[0]), sizes, u32(nums[k]), u32(nums[1]), i32(nums[2]), i32(nums[3])]
        rc = (L.rl_mlp_create_layers(*head, out) if ctor == "mlp_layers" else
              L.rl_mlp_create_config(*head, i32(nums[4]), out))
    elif ctor in ("gru_mlp", "lstm_mlp"):
        fn = L.rl_gru_mlp_create if ctor == "gru_mlp" else L.rl_lstm_mlp_create
        rc = fn(eng.h, u32(nums[0]), u32(nums[1]), u32(nums[2]), u32(nums[3]), out)
    elif ctor == "rnn_mlp":
        rc = L.rl_rnn_mlp_create(eng.h, i32(nums[0]), u32(nums[1]), u32(nums[2]), u32(nums[3]), u32(nums[4]), u32(nums[5]), out)
    elif ctor == "rnn_mlp_config":
        rc = L.rl_rnn_mlp_create_config(eng.h, i32(nums[0]), u32(nums[1]), u32(nums[2]), u32(nums[3]), i32(nums[4]),
                                        u32(nums[5]), u32(nums[6]), out)
    elif ctor == "rnn_linear":
        rc = L.rl_rnn_linear_create(eng.h, i32(nums[0]), u32(nums[1]), u32(nums[2]), u32(nums[3]), i32(nums[4]), u32(nums[5]), out)
    elif ctor in ("chain", "chain_wide"):
        cfg = ra.RnnChainConfig(*nums)
        fn = L.rl_rnn_chain_create if ctor == "chain" else L.rl_rnn_chain_create_wide
        rc = fn(eng.h, C.byref(cfg), out)
    else:
        raise AssertionError(ctor)
    return rc, h, "module"


INIT_MODULES = {0: ("mlp_layers", [4, 1, CC.RELU, CC.IDENTITY, 1, 3]), 1: ("mlp_config", [4, 1, CC.RELU, CC.IDENTITY, 0, 1, 3]),
                2: ("gru_mlp", [4, 3, 3, 1]), 3: ("rnn_mlp_config", [CC.GRU, 4, 3, 1, 0, 3, 1])}


def last_error(eng):
    return ra.lib().rl_last_error(eng.h if eng is not None else None).decode()


def destroy(h, what):
    (ra.lib().rl_env_destroy if what == "env" else ra.lib().rl_mlp_destroy)(h)


def run_case(eng, ctor, nums):
    L = ra.lib()
    if ctor in ("init_mlp", "init_rnn"):
        rc, h, what = create(eng, *INIT_MODULES[nums[0]])
        assert rc == ra.OK, last_error(eng)
        keep, ptrs = initializers(nums[1:])
        rc = (L.rl_mlp_init_with if ctor == "init_mlp" else L.rl_rnn_mlp_init_with)(h, u64(11), *ptrs)
        rec = {"code": rc, "message": last_error(eng)} if rc != ra.OK else {"code": ra.OK}
        destroy(h, what)
        return rec
    bytes0, allocs0 = ra.debug_device_memory()
    rc, h, what = create(eng, ctor, nums)
    bytes1, allocs1 = ra.debug_device_memory()
    rec = {"code": rc, "bytes": bytes1 - bytes0, "allocations": allocs1 - allocs0}
    if rc != ra.OK:
        assert not h, "a refused create leaves *out NULL"
        rec["message"] = last_error(eng)
        return rec
    if what == "env":
        d, a = u32(), u32()
        assert L.rl_env_dims(h, C.byref(d), C.byref(a)) == ra.OK
        rec["dims"] = [d.value, a.value]
    else:
        n = u64()
        assert L.rl_mlp_num_params(h, C.byref(n)) == ra.OK
        rec["params"] = n.value
    destroy(h, what)
    rec["released"] = ra.debug_device_memory() == (bytes0, allocs0)
    return rec


# ---------------------------------------------------------------------- NULL arguments: name -> call(engine) -> (code, engine whose
# error it is or None)
def null_cases():
    L = ra.lib()
    cfg = env_config(ra.ENV_CARTPOLE, ra.LIMIT_VISIBLE, 9, 4)
    meta = ra.MetaBanditConfig(2, 0, 3)
    mdp = ra.TabularMdpConfig(2, 2, 1.0)
    tr, mean, _ = mdp_tables(2, 2, 0)
    trp, meanp = tr.ctypes.data_as(C.c_void_p), mean.ctypes.data_as(C.c_void_p)
    values = (C.c_double * 3)(0.0, 1.0, 2.0)
    chain = ra.RnnChainConfig(0, 5, 8, 1, 1, 8, 2)
    wide = ra.RnnChainConfig(0, 16, 8, 1, 1, 8, 12)
    glorot = ra.Initializer(2, 3, 0.0)
    g, sizes = C.byref(glorot), (u32 * 1)(8)

    def out():
        return C.byref(C.c_void_p())

    def with_module(eng, which, fn):
        rc, h, what = create(eng, *INIT_MODULES[which])
        assert rc == ra.OK
        rc = fn(h)
        destroy(h, what)
        return rc

    return {
        "null-env-config": lambda e: (L.rl_env_create(e.h, None, out()), e),
        "null-env-out": lambda e: (L.rl_env_create(e.h, C.byref(cfg), None), e),
        "null-env-engine": lambda e: (L.rl_env_create(None, C.byref(cfg), out()), None),
        "null-bandit-values": lambda e: (L.rl_env_create_bandit(e.h, C.byref(cfg), None, u32(3), out()), e),
        "null-bandit-config": lambda e: (L.rl_env_create_bandit(e.h, None, values, u32(3), out()), e),
        "null-meta-config": lambda e: (L.rl_env_create_meta_bandit(e.h, C.byref(cfg), None, out()), e),
        "null-meta-wide-config": lambda e: (L.rl_env_create_meta_bandit_wide(e.h, C.byref(cfg), None, out()), e),
        "null-meta-out": lambda e: (L.rl_env_create_meta_bandit_wide(e.h, C.byref(cfg), C.byref(meta), None), e),
        "null-mdp-transitions": lambda e: (L.rl_env_create_tabular_mdp(e.h, C.byref(cfg), C.byref(mdp), None, meanp, None, out()), e),
        "null-mdp-config": lambda e: (L.rl_env_create_tabular_mdp(e.h, C.byref(cfg), None, trp, meanp, None, out()), e),
        "null-mdp-out": lambda e: (L.rl_env_create_tabular_mdp(e.h, C.byref(cfg), C.byref(mdp), trp, meanp, None, None), e),
        "null-mlp-out": lambda e: (L.rl_mlp_create(e.h, u32(5), u32(8), u32(2), None), e),
        "null-mlp-engine": lambda e: (L.rl_mlp_create(None, u32(5), u32(8), u32(2), out()), None),
        "null-layers-sizes": lambda e: (L.rl_mlp_create_layers(e.h, u32(6), None, u32(1), u32(2), i32(1), i32(0), out()), e),
        "null-layers-sizes-fused-shape": lambda e: (L.rl_mlp_create_layers(e.h, u32(5), None, u32(1), u32(2), i32(1), i32(0), out()), e),
        "null-layers-out-fused-shape": lambda e: (L.rl_mlp_create_config(e.h, u32(5), sizes, u32(1), u32(2), i32(1), i32(0), i32(1), None), e),
        "null-gru-mlp-out": lambda e: (L.rl_gru_mlp_create(e.h, u32(5), u32(8), u32(8), u32(2), None), e),
        "null-rnn-linear-out": lambda e: (L.rl_rnn_linear_create(e.h, i32(0), u32(5), u32(8), u32(1), i32(1), u32(2), None), e),
        "null-chain-config": lambda e: (L.rl_rnn_chain_create(e.h, None, out()), e),
        "null-chain-out": lambda e: (L.rl_rnn_chain_create(e.h, C.byref(chain), None), e),
        "null-chain-wide-config": lambda e: (L.rl_rnn_chain_create_wide(e.h, None, out()), e),
        "null-chain-wide-out": lambda e: (L.rl_rnn_chain_create_wide(e.h, C.byref(wide), None), e),
        "null-init-mlp-module": lambda e: (L.rl_mlp_init_with(None, u64(1), g, g), None),
        "null-init-mlp-kernel": lambda e: (with_module(e, 0, lambda h: L.rl_mlp_init_with(h, u64(1), None, g)), e),
        "null-init-rnn-module": lambda e: (L.rl_rnn_mlp_init_with(None, u64(1), g, g, g, g, g), None),
    }


def run_null_case(eng, call):
    before = ra.debug_device_memory()
    rc, whose = call(eng)
    assert ra.debug_device_memory() == before
    return {"code": rc, "message": last_error(whose)}


NULL_NAMES = ["null-env-config", "null-env-out", "null-env-engine", "null-bandit-values", "null-bandit-config",
              "null-meta-config", "null-meta-wide-config", "null-meta-out", "null-mdp-transitions", "null-mdp-config",
              "null-mdp-out", "null-mlp-out", "null-mlp-engine", "null-layers-sizes", "null-layers-sizes-fused-shape",
              "null-layers-out-fused-shape", "null-gru-mlp-out", "null-rnn-linear-out", "null-chain-config",
              "null-chain-out", "null-chain-wide-config", "null-chain-wide-out", "null-init-mlp-module",
              "null-init-mlp-kernel", "null-init-rnn-module"]


def all_names():
    return [name for name, _, _ in CC.CASES] + NULL_NAMES


def run(eng, name):
    nulls = null_cases()
    assert list(nulls) == NULL_NAMES
    if name in nulls:
        return run_null_case(eng, nulls[name])
    ctor, nums = CC.by_name()[name]
    return run_case(eng, ctor, nums)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def engine():
    eng = ra.Engine(0)
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", all_names())
def test_constructor_table(engine, golden, name):
    got = run(engine, name)
    print(name, got)
    assert got == golden[name]
    assert got["code"] != ra.OK or got.get("released", True), "device memory is back where it started after the destroy"
    assert got["code"] == ra.OK or got.get("bytes", 0) == 0 and got.get("allocations", 0) == 0, "a refused create holds nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("wide,narrow", CC.SAME_RECORD)
def test_shorthand_constructors_build_the_same_handle(engine, wide, narrow):
    assert run(engine, wide) == run(engine, narrow)


def test_the_table_covers_the_case_list(golden):
    """(no GPU) every case has a recorded answer and the file holds no others"""
    assert sorted(golden) == sorted(all_names())
    assert len(set(all_names())) == len(all_names())


def record(path):
    eng = ra.Engine(0)
    table = {name: run(eng, name) for name in all_names()}
    eng.close()
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(table), path))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write the table instead of checking it")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if not args.record:
        ap.error("run under pytest to check; --record writes the table")
    record(args.out)
