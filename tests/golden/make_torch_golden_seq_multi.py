"""Golden vectors for recurrent chains over MORE THAN TWO actions — ChainConfig<GruConfig | LstmConfig, MlpConfig |
LinearConfig> with out_dim = 3 and 8 (src/torch/modules/chain.rs:12-56, seq/rnn/mod.rs:20-45) — computed with PyTorch
on the CPU, the library the reference binds through tch.

    python tests/golden/make_torch_golden_seq_multi.py      -> tests/golden/torch_golden_seq_multi.json

Per case (f64): torch.nn.GRU / torch.nn.LSTM (num_layers = L, stepped one observation at a time with the episode state
carried, zero at the start of an episode) -> relu -> torch.nn.Linear (-> relu -> torch.nn.Linear) over lane trajectories
with episode ends inside the history and at the horizon:
  out    the logits [A][T][n]
  grad   the gradient of -mean(adv * ratio), ratio = exp(log pi(a) - log pi_0(a)) at pi = pi_0 (Trpo::update's closure,
         policies/trpo.rs:97-146), by autograd
  fvp    the Fisher-vector product along `v`: d/d theta (grad_theta mean KL(pi_0 || pi) . v) by double backward
         (HessianVectorProduct, conjugate_gradient.rs:262-339), no regularisation term
Flat parameter order = trainable_variables(): per layer [W_ih, W_hh, b_ih, b_hh], then the tail's kernel / bias pairs."""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def seq_multi_case(cell, L, H2, A, D=2, H=4, n=3, T=5, seed=81):
    dtype = torch.float64
    g = torch.Generator().manual_seed(seed)
    rnn = (torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(D, H, num_layers=L).to(dtype)
    tail = [torch.nn.Linear(H, A)] if H2 == 0 else [torch.nn.Linear(H, H2), torch.nn.Linear(H2, A)]
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
    action = torch.randint(0, A, (T, n), generator=g)
    action.view(-1)[:A] = torch.arange(A)[:T * n]  # every index the history has room for occurs
    adv = torch.randn(T, n, generator=g, dtype=dtype)
    v = [torch.randn(t.shape, generator=g, dtype=dtype) for t in tensors]

    def logits():
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
        return torch.stack(rows).reshape(n, T, A).permute(2, 1, 0)  # [A][T][n]

    z = logits()
    lp = torch.log_softmax(z, dim=0)
    lp0 = lp.detach()
    lpa = torch.gather(lp, 0, action.unsqueeze(0))[0]
    loss = -(adv * torch.exp(lpa - lpa.detach())).mean()
    grad = torch.autograd.grad(loss, tensors, retain_graph=True)
    kl = (torch.exp(lp0) * (lp0 - lp)).sum(0).mean()
    gk = torch.autograd.grad(kl, tensors, create_graph=True)
    dot = sum((a * b).sum() for a, b in zip(gk, v))
    fvp = torch.autograd.grad(dot, tensors)
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).tolist()
    return {
        "cell": cell, "dims": [D, H, L, H2, A], "n": n, "T": T, "dtype": "float64",
        "params": flat([t.detach() for t in tensors]), "obs": obs.flatten().tolist(),
        "term_obs": term_obs.flatten().tolist(), "flag": flag.flatten().tolist(), "action": action.flatten().tolist(),
        "adv": adv.flatten().tolist(), "v": flat(v), "out": z.detach().flatten().tolist(), "grad": flat(grad),
        "fvp": flat(fvp),
    }


def main():
    torch.set_num_threads(1)
    cases = {"generator": f"torch {torch.__version__} (CPU), make_torch_golden_seq_multi.py"}
    # the smallest shapes with D, H, H2 and A pairwise different, so that no transposed block passes; A enters the head
    # alone, and each cell with each tail is pinned at A <= 2 by the stacked and chain-linear files
    cases["gru_l1_linear_a3"] = seq_multi_case("gru", 1, 0, 3, seed=81)
    cases["lstm_l2_mlp_a8"] = seq_multi_case("lstm", 2, 5, 8, H=3, seed=83)  # two layers
    with open(os.path.join(HERE, "torch_golden_seq_multi.json"), "w") as f:
        json.dump(cases, f)
    print("wrote torch_golden_seq_multi.json")


if __name__ == "__main__":
    main()
