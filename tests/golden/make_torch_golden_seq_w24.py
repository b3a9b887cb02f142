"""Golden vectors for recurrent chains of 23 and 24 inputs — ChainConfig<GruConfig | LstmConfig, MlpConfig | LinearConfig>
as rl_rnn_chain_create_wide24 builds them: policy (two outputs) and critic (one output) of the partition-game experiment
on PartitionGame lanes (23 features, 24 under a visible step limit) — computed with PyTorch on the CPU, the library the
reference binds through tch.

    python tests/golden/make_torch_golden_seq_w24.py      -> tests/golden/torch_golden_seq_w24.json

Two outputs: make_torch_golden_seq_multi.py's `seq_multi_case` (logits, the gradient of -mean(adv * ratio) and one
Fisher-vector product by double backward, f64).  One output: `seq_value_case` here — the values and the gradient of the
critic's loss mean((V - target)^2); a categorical over one output has no Fisher information, so there is no product to
record.  Five cases: 23 and 24 inputs, two outputs and one, both cells and both tails at each output count, the
experiment's policy (GRU, MLP tail, 24 -> 2) and its critic (24 -> 1) among them."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_torch_golden_seq_multi import seq_multi_case  # noqa: E402


def seq_value_case(cell, L, H2, D, H=4, n=3, T=5, seed=91):
    """seq_multi_case's network, history and episode cuts with one output and the loss mean((V - target)^2)"""
    dtype = torch.float64
    g = torch.Generator().manual_seed(seed)
    rnn = (torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(D, H, num_layers=L).to(dtype)
    tail = [torch.nn.Linear(H, 1)] if H2 == 0 else [torch.nn.Linear(H, H2), torch.nn.Linear(H2, 1)]
    tail = [m.to(dtype) for m in tail]
    tensors = []
    for l in range(L):
        tensors += [getattr(rnn, f"weight_ih_l{l}"), getattr(rnn, f"weight_hh_l{l}"), getattr(rnn, f"bias_ih_l{l}"),
                    getattr(rnn, f"bias_hh_l{l}")]
    for m in tail:
        tensors += [m.weight, m.bias]
    with torch.no_grad():
        for t in tensors:
            t.copy_((torch.rand(t.shape, generator=g, dtype=dtype) * 2 - 1) * 0.7)
    obs = torch.randn(D, T + 1, n, generator=g, dtype=dtype)
    term_obs = torch.randn(D, T, n, generator=g, dtype=dtype)
    flag = torch.zeros(T, n, dtype=torch.int64)
    flag[1, 0] = 1   # Terminate
    flag[3, 0] = 2   # Interrupt
    flag[2, 1] = 2
    flag[T - 1, 2] = 1  # at the horizon
    target = torch.randn(T, n, generator=g, dtype=dtype)

    rows = []
    for i in range(n):
        st = None  # zero state
        for t in range(T):
            y, st = rnn(obs[:, t, i].reshape(1, 1, D), st)
            y = torch.relu(y.reshape(H))
            for k, m in enumerate(tail):
                y = m(y) if k == len(tail) - 1 else torch.relu(m(y))
            rows.append(y)
            if int(flag[t, i]) != 0:
                st = None
    z = torch.stack(rows).reshape(n, T, 1).permute(2, 1, 0)  # [1][T][n]
    loss = ((z[0] - target) ** 2).mean()
    grad = torch.autograd.grad(loss, tensors)
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).tolist()
    return {
        "cell": cell, "dims": [D, H, L, H2, 1], "n": n, "T": T, "dtype": "float64",
        "params": flat([t.detach() for t in tensors]), "obs": obs.flatten().tolist(),
        "term_obs": term_obs.flatten().tolist(), "flag": flag.flatten().tolist(), "target": target.flatten().tolist(),
        "out": z.detach().flatten().tolist(), "loss": float(loss.detach()), "grad": flat(grad),
    }


def main():
    torch.set_num_threads(1)
    cases = {"generator": f"torch {torch.__version__} (CPU), make_torch_golden_seq_w24.py"}
    # H and H2 stay small: two recurrent units and three hidden ones keep the file small; every block carries gradient
    cases["gru_l1_mlp_d24_a2"] = seq_multi_case("gru", 1, 3, 2, D=24, H=2, seed=111)  # the experiment's policy
    cases["lstm_l1_linear_d23_a2"] = seq_multi_case("lstm", 1, 0, 2, D=23, H=2, seed=112)
    cases["gru_l1_mlp_d24_a1"] = seq_value_case("gru", 1, 3, D=24, H=2, seed=115)  # the experiment's critic
    cases["lstm_l1_mlp_d24_a1"] = seq_value_case("lstm", 1, 3, D=24, H=2, seed=116)
    cases["gru_l1_linear_d23_a1"] = seq_value_case("gru", 1, 0, D=23, H=2, seed=117)
    with open(os.path.join(HERE, "torch_golden_seq_w24.json"), "w") as f:
        json.dump(cases, f)
    print("wrote torch_golden_seq_w24.json")


if __name__ == "__main__":
    main()
