"""rl_env_create_bandit and the widened module / MemoryGame sizes, as far as they can be checked without a device: the
symbol is declared, exported, bound and documented, the ABI version is unchanged, and the argument checks that run before
any device work answer with their status codes.  CPU only."""
import ctypes as C
import os
import re

import relearn_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_symbol_is_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "relearn_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int32_t rl_env_create_bandit\(rl_engine \*engine, const rl_env_config \*cfg, "
                  r"const double \*values,\s*uint32_t n_arms,\s*rl_env \*\*out\);", header, re.S)
    assert m, "prototype with its comment"
    assert "src/envs/bandits.rs:109-116" in m.group(1)  # DeterministicBandit::from_values
    assert "rl_env_create_bandit" in ra.ABI_SYMBOLS
    ra.build()
    assert hasattr(ra.lib(), "rl_env_create_bandit")
    assert ra.lib().rl_abi_version() == 6 and "#define RL_ABI_VERSION 6" in header
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn rl_env_create_bandit(" in doc


def test_env_config_layout_is_unchanged():
    """rl_env_config is pinned by ABI 6: more than two arms go through the new entry point, not through the struct"""
    assert ra.EnvConfig.bandit_values.size == 2 * C.sizeof(C.c_double)
    assert C.sizeof(ra.EnvConfig) == 8 + 5 * 8 + 11 * 8 + 3 * 8 + 16
    header = open(os.path.join(ROOT, "include", "relearn_hip.h")).read()
    assert "double bandit_values[2];" in header


def test_null_arguments_are_refused_without_a_device():
    ra.build()
    L = ra.lib()
    cfg = ra.EnvConfig()
    cfg.kind, cfg.n_lanes = ra.ENV_BANDIT, 32
    values = (C.c_double * 4)(0.0, 0.0, 0.0, 1.0)
    out = C.c_void_p()
    assert L.rl_env_create_bandit(None, C.byref(cfg), values, C.c_uint32(4), C.byref(out)) == ra.ERR_INVALID_ARGUMENT
    assert L.rl_env_create_bandit(None, C.byref(cfg), None, C.c_uint32(4), C.byref(out)) == ra.ERR_INVALID_ARGUMENT
    assert not out
    sizes = (C.c_uint32 * 1)(32)
    assert L.rl_mlp_create_layers(None, C.c_uint32(7), sizes, C.c_uint32(1), C.c_uint32(3), C.c_int32(1), C.c_int32(0),
                                  C.byref(out)) == ra.ERR_INVALID_ARGUMENT
