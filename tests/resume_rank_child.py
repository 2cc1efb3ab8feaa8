"""One rank of a two-rank ``train(resume=True)`` job (test infrastructure): started by tests/test_gpu_resume.py as
a FRESH interpreter with RANK / WORLD_SIZE / MASTER_* in the environment.  ``argv``: the directory for this
phase's records, the directory under which rank r keeps ``rank<r>/`` as its checkpoint directory, and the step at
whose evaluation every rank raises (0: none).  Writes what the logger received to <out_dir>/rank<r>.json, also
when it is cut."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_dir, ckpt_base, cut_at = sys.argv[1], sys.argv[2], int(sys.argv[3])
    rank = int(os.environ.get("RANK", "0"))
    import iqlpref_amd as ia
    S, A, n = 5, 3, 300
    rng = np.random.default_rng(5)
    data = {"observations": rng.standard_normal((n, S)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
            "rewards": rng.uniform(size=n).astype(np.float32),
            "next_observations": rng.standard_normal((n, S)).astype(np.float32),
            "terminals": (rng.uniform(size=n) < 0.05).astype(np.float32)}
    cfg = ia.TrainConfig(env="resume-fake-v0", seed=100, max_timesteps=40, log_freq=4, eval_freq=10, batch_size=16,
                         hidden_dim=64, actor_dropout=0.1, device="cuda", checkpoints_path=ckpt_base)
    # (a config made anew draws a new random name: the run's own directory is set by hand, one per rank)
    cfg.name, cfg.checkpoints_path = "two-ranks", os.path.join(ckpt_base, f"rank{rank}")
    logs = []

    def evaluate(actor, t):
        if t == cut_at:
            raise RuntimeError(f"cut in the evaluation at step {t}")
        return np.array([float(actor.net.linears()[2].weight.detach().double().sum())]), [t]

    trainers = []
    try:
        trainers = ia.train(cfg, dataset=data, state_dim=S, action_dim=A, max_action=1.0, precision="bf16",
                            logger=lambda rec, step: logs.append([int(step), {k: float(v) for k, v in rec.items()
                                                                              if not k.startswith("steps_per_sec")}]),
                            evaluate=evaluate, seeds_per_gpu=2, resume=True)
    finally:
        with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
            json.dump({"rank": rank, "seeds": [t._seed for t in trainers], "total_it": [t.total_it for t in trainers],
                       "logs": logs, "param_sum": [float(t._params.double().sum()) for t in trainers]}, f)
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
