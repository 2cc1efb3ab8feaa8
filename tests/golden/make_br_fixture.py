#!/usr/bin/env python3
"""Generate tests/golden/br_relabel.npz and tests/golden/br_train_run.npz by RUNNING the reference's
Bayesian-reward flavour (algorithms/custom_offline/iql_br.py, "bref") on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_br_fixture.py [--ref /root/reference]

bref is imported under the inert stubs of ``make_fixtures.import_custom_reference`` plus stubs for the
absent ``optbnn`` submodule; its own ``posterior_sampler``, ``qlearning_dataset`` and ``train`` then run
as written.  The BNN is ``tests/br_env.NumpyPosterior``: S small numpy MLPs regenerated from a seed.
Only inputs and outputs are stored: seeds, the [S, N] prediction matrices, the samples / rewards, the
state of numpy's global generator afterwards, and for ``train`` what make_custom_train_fixture.py
stores.  The ``idx`` arrays are derived, not reference output: the indices of ONE
``randint(0, S, size=(N, n))`` from the same seed, stored only after this script has checked that they
reproduce the reference's samples and final state exactly.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import br_env  # noqa: E402
from tests import custom_train_env as cte  # noqa: E402
from tests.golden import make_fixtures  # noqa: E402
from tests.golden.make_custom_train_fixture import COMMON, checkpoint_arrays  # noqa: E402

POST_SEED, MAP_SEED = 40, 900
# (S, n_samps, seed): S = 64 never rejects a word, 65 and 129 reject nearly half of them
SAMPLER_CASES = [(64, 1, 1), (64, 7, 2), (64, 10, 3), (65, 1, 4), (65, 7, 5), (65, 10, 6), (129, 1, 7),
                 (129, 33, 8), (129, 100, 9), (2, 5, 10)]
# (reward_type, n_samples, seed) on the S = 65 posterior
DATASET_CASES = [(0, None, 11), (1, 10, 12), (1, 7, 13), (2, 7, 14), (2, 10, 15), (3, None, 16), (7, None, 17)]
# the train() run: median of 10 draws; normalized score = a + b * returns with b < 0, so that the best
# step by mean return (what bref keeps) and by normalized score (what cref would keep) differ
TRAIN = dict(train_seed=3, relabel_seed=21, reward_type=2, n_samples=10, n_post=65, affine=(50.0, -0.5))


def import_bref(ref_root):
    make_fixtures.import_custom_reference(ref_root)  # installs the stubs of the absent packages

    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m

    stub("optbnn")
    stub("optbnn.bnn")
    stub("optbnn.bnn.likelihoods", LikCE=None)
    stub("optbnn.bnn.nets")
    stub("optbnn.bnn.nets.mlp", MLP=None)
    stub("optbnn.bnn.priors", FixedGaussianPrior=None, OptimGaussianPrior=None)
    stub("optbnn.sgmcmc_bayes_net")
    stub("optbnn.sgmcmc_bayes_net.pref_net", PrefNet=None)
    stub("optbnn.utils", util=None)
    path = os.path.join(ref_root, "algorithms", "custom_offline", "iql_br.py")
    spec = importlib.util.spec_from_file_location("ref_custom_iql_br", path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    keep_path = list(sys.path)
    spec.loader.exec_module(mod)
    sys.path[:] = keep_path
    return mod


def state_arrays(prefix):
    st = np.random.get_state()
    return {f"{prefix}/np_key": np.asarray(st[1], np.uint32), f"{prefix}/np_pos": np.int64(st[2])}


def relabel_fixture(bref):
    c = COMMON
    dataset = cte.MinariDataset(c["data_seed"], c["lengths"])
    env = dataset.recover_environment()
    out = {"data_seed": np.int64(c["data_seed"]), "lengths": np.asarray(c["lengths"]),
           "post_seed": np.int64(POST_SEED), "map_seed": np.int64(MAP_SEED), "hidden": np.int64(br_env.HIDDEN)}
    sets = br_env.posterior_layers(POST_SEED, 129, env.S, env.A)
    map_set = br_env.posterior_layers(MAP_SEED, 1, env.S, env.A)[0]
    all_preds = br_env.predictions_of(sets, dataset)  # (per episode, as bref's loop asks for them)
    preds = {S: np.ascontiguousarray(all_preds[:S]) for S in (2, 64, 65, 129)}
    for S, p in preds.items():
        out[f"preds/{S}"] = p
    out["map_preds"] = br_env.predictions_of([map_set], dataset)[0]
    for S, n, seed in SAMPLER_CASES:
        tag = f"sampler/S{S}_n{n}"
        np.random.seed(seed)
        samples = np.asarray(bref.posterior_sampler(preds[S].T, n))  # [N, n]
        out[f"{tag}/seed"], out[f"{tag}/samples"] = np.int64(seed), samples
        out.update(state_arrays(tag))
        np.random.seed(seed)
        mine, idx = br_env.posterior_sampler(preds[S], n)
        assert mine.tobytes() == samples.reshape(mine.shape).tobytes(), tag
        mine_state = np.random.get_state()
        assert (mine_state[1] == out[f"{tag}/np_key"]).all() and mine_state[2] == out[f"{tag}/np_pos"], tag
        out[f"{tag}/idx"] = idx.astype(np.uint16)
    model = br_env.NumpyPosterior(sets[:65], map_set)
    for rtype, n, seed in DATASET_CASES:
        tag = f"dataset/type{rtype}_n{n}"
        np.random.seed(seed)
        d = bref.qlearning_dataset(dataset, model, rtype, n)
        out[f"{tag}/seed"] = np.int64(seed)
        out[f"{tag}/rewards"] = np.asarray(d["rewards"])
        for k in ("observations", "actions", "next_observations", "terminals"):
            out[f"{tag}/{k}/sum"] = np.float64(np.asarray(d[k], np.float64).sum())
            out[f"{tag}/{k}/shape"] = np.asarray(d[k].shape)
        out.update(state_arrays(tag))
    cfg = bref.TrainConfig()
    out["config/fields"] = np.asarray(sorted(vars(cfg)))
    for k, v in vars(cfg).items():
        if k not in ("name",):
            out[f"config/default/{k}"] = np.asarray("None" if v is None else v)
    opt = bref.TrainConfig(use_optim_prior=True, reward_model_path="/m", mapper_num_iters=7, checkpoints_path="/c")
    out["config/optim/saved_dir"], out["config/optim/ckpt_path"] = np.asarray(opt.saved_dir), np.asarray(opt.ckpt_path)
    out["config/optim/checkpoints_dir"] = np.asarray(os.path.dirname(opt.checkpoints_path))
    out["config/std/saved_dir"] = np.asarray(bref.TrainConfig(reward_model_path="/m").saved_dir)
    return out


def train_fixture(bref):
    c, t = COMMON, TRAIN
    dataset = cte.MinariDataset(c["data_seed"], c["lengths"])
    env = dataset.recover_environment()
    sets = br_env.posterior_layers(POST_SEED, t["n_post"], env.S, env.A)
    records, saves = [], []

    def log(d, step):
        for k, v in d.items():
            records.append((int(step), k, float(v)))

    affine = t["affine"]
    bref.wandb = types.SimpleNamespace(init=lambda **kw: None, log=log)
    bref.minari = types.SimpleNamespace(download_dataset=lambda i: None, load_dataset=lambda i: dataset,
                                        get_normalized_score=lambda ds, r: affine[0] + affine[1] * np.asarray(r))
    bref.pyrallis = types.SimpleNamespace(dump=lambda cfg, f: f.write(repr(cfg)))
    bref.FixedGaussianPrior = lambda std: None
    bref.MLP = lambda *a: None
    bref.LikCE = lambda: None
    bref.PrefNet = lambda net, lik, prior, saved_dir, n_gpu: br_env.NumpyPosterior(sets)
    real_save = torch.save

    def save(obj, path):
        saves.append((records[-1][0], os.path.basename(path)))
        real_save(obj, path)

    with tempfile.TemporaryDirectory() as tmp:
        config = bref.TrainConfig(update_steps=c["update_steps"], eval_every=c["eval_every"],
                                  batch_size=c["batch_size"], eval_episodes=c["eval_episodes"],
                                  eval_seed=c["eval_seed"], train_seed=t["train_seed"], checkpoints_path=tmp,
                                  reward_type=t["reward_type"], n_samples=t["n_samples"])
        np.random.seed(t["relabel_seed"])  # the relabel runs before set_seed(train_seed)
        torch.save = save
        try:
            bref.train(config)
        finally:
            torch.save = real_save
        state = np.random.get_state()
        last = max((s for s in saves if s[1].startswith("checkpoint_")), key=lambda s: s[0])[1]
        best = torch.load(os.path.join(config.checkpoints_path, "best_model.pt"), weights_only=True)
        final = torch.load(os.path.join(config.checkpoints_path, last), weights_only=True)
    # the two best-model rules part on this run: recorded, and checked here
    ret = [(s, v) for s, k, v in records if k == "evaluation_return"]
    nrm = [(s, v) for s, k, v in records if k == "normalized_score"]
    by_return = max(ret, key=lambda r: r[1])[0]
    by_norm = max(nrm, key=lambda r: r[1])[0]
    assert by_return != by_norm, "pick another affine map: both rules keep the same step"
    assert [v for s, k, v in records if k == "best_step_so_far"][-1] == by_return
    out = {k: np.asarray(v) for k, v in t.items()}
    out.update({"post_seed": np.int64(POST_SEED), "hidden": np.int64(br_env.HIDDEN),
                "best_by_return": np.int64(by_return), "best_by_normalized": np.int64(by_norm),
                "preds": br_env.predictions_of(sets, dataset),
                "rec_step": np.asarray([r[0] for r in records], np.int64),
                "rec_key": np.asarray([r[1] for r in records]),
                "rec_value": np.asarray([r[2] for r in records], np.float64),
                "save_step": np.asarray([s[0] for s in saves], np.int64),
                "save_name": np.asarray([s[1] for s in saves]),
                "np_key": np.asarray(state[1], np.uint32), "np_pos": np.int64(state[2]),
                "np_has_gauss": np.int64(state[3]), "np_cached": np.float64(state[4])})
    out.update({f"common/{k}": np.asarray(v) for k, v in c.items()})
    out.update(checkpoint_arrays("best", best))
    out.update(checkpoint_arrays("last", final))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    bref = import_bref(args.ref)
    torch.set_num_threads(1)  # (the CPU reference's reductions in one fixed order)
    for name, arrays in (("br_relabel.npz", relabel_fixture(bref)), ("br_train_run.npz", train_fixture(bref))):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
