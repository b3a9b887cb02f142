"""Golden vectors for recurrent chains with a Linear tail, ChainConfig<GruConfig | LstmConfig, LinearConfig>
(src/torch/modules/chain.rs:12-54, ff/linear.rs:13-68), computed with PyTorch on the CPU — the library the reference
binds through tch.

    python tests/golden/make_torch_golden_chain_linear.py      -> tests/golden/torch_golden_chain_linear.json

Per case (f64): torch.nn.GRU / torch.nn.LSTM (num_layers = L, stepped one observation at a time with the episode state
carried, zero at the start of an episode) -> relu -> torch.nn.Linear over lane trajectories with episode ends inside the
history — per-step outputs, successor outputs at cut episodes, and the gradient of sum(dout * out) through time by
autograd.  Flat parameter order = trainable_variables(): per layer [W_ih, W_hh, b_ih, b_hh], then kernel [A, H],
bias [A]."""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def chain_linear_case(cell, L, D=6, H=7, A=2, n=3, T=5, seed=71):
    dtype = torch.float64
    g = torch.Generator().manual_seed(seed)
    rnn = (torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(D, H, num_layers=L).to(dtype)
    lin = torch.nn.Linear(H, A).to(dtype)
    tensors = []
    for l in range(L):
        tensors += [getattr(rnn, f"weight_ih_l{l}"), getattr(rnn, f"weight_hh_l{l}"), getattr(rnn, f"bias_ih_l{l}"),
                    getattr(rnn, f"bias_hh_l{l}")]
    tensors += [lin.weight, lin.bias]
    with torch.no_grad():
        for t in tensors:
            t.copy_((torch.rand(t.shape, generator=g, dtype=dtype) * 2 - 1) * 0.7)
    obs = torch.randn(D, T + 1, n, generator=g, dtype=dtype)
    term_obs = torch.randn(D, T, n, generator=g, dtype=dtype)
    flag = torch.zeros(T, n, dtype=torch.int64)
    flag[1, 0] = 1   # Terminate
    flag[3, 0] = 2   # Interrupt
    flag[2, 1] = 2
    flag[T - 1, 2] = 1
    dout = torch.randn(A, T, n, generator=g, dtype=dtype)

    def step(x, st):  # x [D] -> (module output [A], new state)
        y, st = rnn(x.reshape(1, 1, D), st)
        return lin(torch.relu(y.reshape(H))), st

    out = torch.zeros(A, T, n, dtype=dtype)
    succ = torch.zeros(A, T, n, dtype=dtype)
    loss = 0
    for i in range(n):
        st = None  # zero state
        for t in range(T):
            y, st = step(obs[:, t, i], st)
            out[:, t, i] = y.detach()
            loss = loss + (dout[:, t, i] * y).sum()
            f = int(flag[t, i])
            if f == 2 or (f == 0 and t == T - 1):
                succ[:, t, i] = step(term_obs[:, t, i] if f == 2 else obs[:, T, i], st)[0].detach()
            if f != 0:
                st = None
    loss.backward()
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).tolist()
    return {
        "cell": cell, "dims": [D, H, L, A], "n": n, "T": T, "dtype": "float64",
        "params": flat([t.detach() for t in tensors]), "obs": obs.flatten().tolist(),
        "term_obs": term_obs.flatten().tolist(), "flag": flag.flatten().tolist(), "dout": dout.flatten().tolist(),
        "out": out.flatten().tolist(), "succ_out": succ.flatten().tolist(), "grad": flat([t.grad for t in tensors]),
    }


def main():
    torch.set_num_threads(1)
    cases = {"generator": f"torch {torch.__version__} (CPU), make_torch_golden_chain_linear.py"}
    cases["gru_l1"] = chain_linear_case("gru", 1, seed=71)
    cases["gru_l2"] = chain_linear_case("gru", 2, seed=73)
    cases["lstm_l2"] = chain_linear_case("lstm", 2, seed=75)
    with open(os.path.join(HERE, "torch_golden_chain_linear.json"), "w") as f:
        json.dump(cases, f)
    print("wrote torch_golden_chain_linear.json")


if __name__ == "__main__":
    main()
