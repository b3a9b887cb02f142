"""Golden vectors for recurrent chains of 19 and 20 inputs — ChainConfig<GruConfig | LstmConfig, MlpConfig | LinearConfig>
as rl_rnn_chain_create_wide20 builds them: the RL2 experiment's model on random MDPs of 10 states and 5 actions
(D = S + A + 4 = 19) and the widest lanes (D = 20, eight actions) — computed with PyTorch on the CPU, the library the
reference binds through tch.

    python tests/golden/make_torch_golden_seq_xwide.py      -> tests/golden/torch_golden_seq_xwide.json

The cases are make_torch_golden_seq_multi.py's (its `seq_multi_case`: logits, the gradient of -mean(adv * ratio) and one
Fisher-vector product by double backward, f64) at (D, A) = (19, 5) and (20, 8), each with a Linear tail and an MLP tail,
both cells, one case of two layers."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_torch_golden_seq_multi import seq_multi_case  # noqa: E402


def main():
    torch.set_num_threads(1)
    cases = {"generator": f"torch {torch.__version__} (CPU), make_torch_golden_seq_xwide.py"}
    # H and H2 stay small and different from D and A
    cases["gru_l1_linear_d19_a5"] = seq_multi_case("gru", 1, 0, 5, D=19, H=4, seed=101)
    cases["lstm_l1_mlp_d19_a5"] = seq_multi_case("lstm", 1, 6, 5, D=19, H=3, seed=102)
    cases["lstm_l2_linear_d20_a8"] = seq_multi_case("lstm", 2, 0, 8, D=20, H=3, seed=103)  # two layers
    cases["gru_l1_mlp_d20_a8"] = seq_multi_case("gru", 1, 6, 8, D=20, H=4, seed=104)
    with open(os.path.join(HERE, "torch_golden_seq_xwide.json"), "w") as f:
        json.dump(cases, f)
    print("wrote torch_golden_seq_xwide.json")


if __name__ == "__main__":
    main()
