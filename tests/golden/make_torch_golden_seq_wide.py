"""Golden vectors for the WIDE recurrent chains — ChainConfig<GruConfig | LstmConfig, MlpConfig | LinearConfig> with more
than eight inputs and outputs (rl_rnn_chain_create_wide: the RL2 bandit experiment's model on 9 and 12 arms, D = k + 4) —
computed with PyTorch on the CPU, the library the reference binds through tch.

    python tests/golden/make_torch_golden_seq_wide.py      -> tests/golden/torch_golden_seq_wide.json

The cases are make_torch_golden_seq_multi.py's (its `seq_multi_case`: logits, the gradient of -mean(adv * ratio) and one
Fisher-vector product by double backward, f64) at (D, A) = (13, 9) and (16, 12), each with a Linear tail and an MLP
tail, both cells, one case of two layers."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_torch_golden_seq_multi import seq_multi_case  # noqa: E402


def main():
    torch.set_num_threads(1)
    cases = {"generator": f"torch {torch.__version__} (CPU), make_torch_golden_seq_wide.py"}
    # H and H2 stay small and different from D and A; n * T = 15 samples hold every action index up to 12
    cases["gru_l1_linear_d13_a9"] = seq_multi_case("gru", 1, 0, 9, D=13, H=4, seed=91)
    cases["lstm_l1_mlp_d13_a9"] = seq_multi_case("lstm", 1, 5, 9, D=13, H=3, seed=92)
    cases["lstm_l2_linear_d16_a12"] = seq_multi_case("lstm", 2, 0, 12, D=16, H=3, seed=93)  # two layers
    cases["gru_l1_mlp_d16_a12"] = seq_multi_case("gru", 1, 5, 12, D=16, H=4, seed=94)
    with open(os.path.join(HERE, "torch_golden_seq_wide.json"), "w") as f:
        json.dump(cases, f)
    print("wrote torch_golden_seq_wide.json")


if __name__ == "__main__":
    main()
