"""The ``algorithms/custom_offline/iql_br.py`` flavour: IQL on Minari episodes whose rewards come from a
BNN posterior over reward networks.  "bref:" = that file; "cref:" = ``custom_offline/iql.py``.

It is the custom flavour with two differences, which ``custom_offline._train`` takes as arguments:

* the relabel (bref:179-253).  S posterior networks predict every transition, and the reward is
  ``reward_type`` 0: one posterior draw, 1: the mean and 2: the median of ``n_samples`` draws, 3: the
  MAP network's prediction.  The draws are ``np.random.choice(row, n)`` once per transition on numpy's
  global legacy generator, which for a 1-D row of length S is ``row[randint(0, S, n)]``; N consecutive
  calls are one ``randint(0, S, size=(N, n))`` stream.  ``iqlhip_posterior_choice`` draws that stream
  on the device (the code of ``iqlhip_np_randint``), gathers from the [S, N] prediction matrix and
  reduces, chunk by chunk; the advanced state goes back into the generator, so afterwards
  ``np.random.get_state()`` is what the reference would have left, bit for bit;
* the best-model rule of ``train`` compares the mean evaluation return only (the normalized-score
  branch is commented out at bref:754-763; the score is still logged).

Not built: ``find_map`` (reward-model training), the fit of ``OptimGaussianPrior`` and the Orbax
readers.  ``PrefNet._load_all_sampled_weights`` lives in the absent ``optbnn`` submodule, so the
directory layout ``PosteriorRewardNet.from_saved_dir`` reads is an ASSUMPTION taken from the offline
flavour's BNN path (ref:899-915).
"""
import ctypes as C
import glob as _glob
import os
import uuid
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import custom_offline as _co
from ._lib import check, ptr
from .custom_offline import (  # noqa: F401  (the rest of the module surface is the custom flavour's)
    ImplicitQLearning, ReplayBuffer, evaluate, modify_reward, pack_np_state, return_reward_range, unpack_np_state)
from .iql import mlp_forward_f32
from .relabel import load_bnn_weight_file

MEAN, MEDIAN = _lib.CHOICE_MEAN, _lib.CHOICE_MEDIAN
MAX_S, MAX_N_SAMPS = 2400, 1024  # the envelope of iqlhip_posterior_choice
TRANSFER_FNS = {"relu": 0, "tanh": 1}  # hidden activation codes of iqlhip_mlp_forward


@dataclass
class TrainConfig:
    """bref:47-103, same fields and defaults; ``saved_dir`` / ``ckpt_path`` are derived."""
    project: str = "IQL-pref"
    group: str = "IQL-Minari-pref"
    name: str = "iql-br"
    gamma: float = 0.99
    tau: float = 0.005
    beta: float = 3.0
    iql_tau: float = 0.7
    iql_deterministic: bool = False
    vf_lr: float = 3e-4
    qf_lr: float = 3e-4
    actor_lr: float = 3e-4
    actor_dropout: Optional[float] = None
    dataset_id: str = "D4RL/pen/human-v2"
    update_steps: int = int(1e6)
    buffer_size: int = 2_000_000
    batch_size: int = 256
    normalize_state: bool = True
    normalize_reward: bool = False
    eval_every: int = int(5e3)
    eval_episodes: int = 10
    train_seed: int = 0
    eval_seed: int = 0
    checkpoints_path: Optional[str] = None
    reward_model_path: str = "./gp_reward-priors/exp/reward_learning/pen/br-pen-f86cc2a5"
    width: int = 64
    depth: int = 3
    transfer_fn: str = "relu"
    mapper_num_iters: int = 1000
    reward_type: int = 0  # 0: posterior draw, 1: predictive mean, 2: predictive median, 3: MAP prediction
    n_samples: Optional[int] = None  # draws per transition of types 1 and 2
    use_optim_prior: bool = False
    map_data: Optional[str] = None

    def __post_init__(self):
        self.name = f"{self.name}-{self.dataset_id}-{str(uuid.uuid4())[:8]}"
        if self.checkpoints_path is not None:
            self.checkpoints_path = os.path.join(self.checkpoints_path, self.name)
        if self.use_optim_prior:
            self.saved_dir = os.path.join(self.reward_model_path, "sampling_optim")
            self.ckpt_path = os.path.join(self.reward_model_path, "ckpts", f"it-{self.mapper_num_iters}.ckpt")
        else:
            self.saved_dir = os.path.join(self.reward_model_path, "sampling_std")


# --------------------------------------------------------------------------- #
# the posterior reward model
# --------------------------------------------------------------------------- #
class PosteriorRewardNet:
    """S posterior weight sets of one reward MLP (and optionally the MAP weight set) on the device.

    A weight set is the list the BNN sampler stores: ``[W0, b0, W1, b1, ...]`` with ``W`` [in, out].
    ``predictions`` fills the device [S, N] matrix with one exact-fp32 ``mlp_forward_f32`` per set, as
    ``relabel._ensemble_rewards`` fills its matrix."""

    def __init__(self, weight_sets: Sequence[Sequence], map_weights: Optional[Sequence] = None,
                 transfer_fn: str = "relu", device: str = "cuda:0"):
        if transfer_fn not in TRANSFER_FNS:
            raise ValueError(f"transfer_fn must be among {tuple(TRANSFER_FNS)}")
        if len(weight_sets) < 1:
            raise ValueError("no posterior weight set")
        self.device = _lib.require_gpu(device)
        self.hidden_act = TRANSFER_FNS[transfer_fn]
        self.sets = [self._upload(w) for w in weight_sets]
        self.map_set = self._upload(map_weights) if map_weights is not None else None

    def _upload(self, w):
        t = [torch.as_tensor(np.asarray(a), dtype=torch.float32, device=self.device) for a in w]
        return t[0::2], t[1::2]

    @property
    def n_posterior(self) -> int:
        return len(self.sets)

    @classmethod
    def from_saved_dir(cls, saved_dir: str, transfer_fn: str = "relu", device: str = "cuda:0",
                       map_weights: Optional[Sequence] = None) -> "PosteriorRewardNet":
        """Every weight set of ``saved_dir/chain_*/sampled_weights/sampled_weights_0000000``, chains in
        sorted order, read with the weights-only loader.  ``saved_dir`` is ``TrainConfig.saved_dir``
        (``sampling_std`` or ``sampling_optim`` under the reward model's directory).  ASSUMED layout:
        the reference reads these files through ``PrefNet._load_all_sampled_weights`` of the absent
        ``optbnn`` submodule; the layout here is the one its offline flavour's BNN path reads
        (ref:899-915)."""
        files = sorted(_glob.glob(os.path.join(saved_dir, "chain_*", "sampled_weights", "sampled_weights_0000000")))
        if not files:
            raise FileNotFoundError(f"No BNN posterior weight files found under {saved_dir}. Expected structure: "
                                    "chain_*/sampled_weights/sampled_weights_0000000")
        sets = []
        for f in files:
            sets.extend(load_bnn_weight_file(f)["sampled_weights"])
        if not sets:
            raise RuntimeError(f"BNN checkpoint at {saved_dir} contained no sampled weights.")
        return cls(sets, map_weights, transfer_fn, device)

    def _x(self, obs_act) -> torch.Tensor:
        return torch.as_tensor(np.asarray(obs_act, np.float32) if not torch.is_tensor(obs_act) else obs_act,
                               dtype=torch.float32, device=self.device)

    def predictions(self, obs_act) -> torch.Tensor:
        """[N, S + A] -> device fp32 [S, N]: row s = the predictions of posterior network s."""
        x = self._x(obs_act)
        out = torch.empty((len(self.sets), x.shape[0]), dtype=torch.float32, device=self.device)
        for k, (ws, bs) in enumerate(self.sets):
            out[k] = mlp_forward_f32(ws, bs, x, w_in_out=True, hidden_act=self.hidden_act)[:, 0]
        return out

    def map_predictions(self, obs_act) -> torch.Tensor:
        """[N, S + A] -> device fp32 [N] from the MAP weight set."""
        if self.map_set is None:
            _map_missing()
        ws, bs = self.map_set
        return mlp_forward_f32(ws, bs, self._x(obs_act), w_in_out=True, hidden_act=self.hidden_act)[:, 0]


def _map_missing():
    raise NotImplementedError(
        "custom_offline_br: reward_type 3 relabels with the MAP network, which the reference finds by training "
        "(PrefNet.find_map on config.map_data); iqlpref_amd has no reward-model training: pass reward_model= a "
        "PosteriorRewardNet holding its parameters (map_weights=)")


# --------------------------------------------------------------------------- #
# the draw (bref:179-186)
# --------------------------------------------------------------------------- #
def posterior_choice(preds: torch.Tensor, n_samps: int, mode: int = MEAN, rng=None, *,
                     return_indices: bool = False):
    """``iqlhip_posterior_choice`` on the generator ``rng`` (an ``np.random.RandomState``; None = numpy's
    global one).  ``preds``: device fp32 [S, N].  Returns the device [N] reduction of ``n_samps`` draws
    per transition (and the uint16-valued [N, n_samps] indices, as int16 storage, when asked: tests).
    The generator's state is uploaded, advanced on the device and written back with ``set_state``."""
    lib = _lib.load()
    if not torch.is_tensor(preds) or preds.dim() != 2:
        raise ValueError("preds must be a device tensor [S, N]")
    S, N, n = int(preds.shape[0]), int(preds.shape[1]), int(n_samps)
    if not 2 <= S <= MAX_S:
        raise ValueError(f"S = {S} posterior predictions per transition: 2..{MAX_S}")
    if not 1 <= n <= MAX_N_SAMPS:
        raise ValueError(f"n_samps = {n}: 1..{MAX_N_SAMPS}")
    if N < 1:
        raise ValueError("no transition")
    if mode not in (MEAN, MEDIAN):
        raise ValueError("mode must be MEAN or MEDIAN")
    dev = _lib.require_gpu(preds.device)
    preds = preds.to(torch.float32).contiguous()
    gen = np.random if rng is None else rng
    before = gen.get_state(legacy=True)
    state = torch.from_numpy(pack_np_state(before).view(np.int32)).to(dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    idx = torch.empty((N, n), dtype=torch.int16, device=dev) if return_indices else None
    nbytes = C.c_size_t(0)
    check(lib.iqlhip_posterior_choice_workspace_bytes(S, N, n, C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.iqlhip_posterior_choice(ptr(state), ptr(preds), S, N, n, int(mode), ptr(out), ptr(idx), ptr(ws),
                                          nbytes.value, _lib.stream_ptr()))
        after = state.cpu().numpy()  # (orders behind the call on the current stream, and waits for it)
        torch.cuda.current_stream().synchronize()  # the workspace may go now
    gen.set_state(unpack_np_state(after, before))
    return (out, idx) if return_indices else out


def posterior_sampler(preds: torch.Tensor, n_samps: int, rng=None) -> torch.Tensor:
    """bref:179-186 with its result materialised: device [N, n_samps] samples, row c drawn from
    ``preds[:, c]``.  NOTE the layout: ``preds`` is the device [S, N] matrix ``predictions`` returns (the
    reference takes its transpose, [N, S]).  The draw is the device stream; the gather by the full
    index matrix is a torch op -- this mirror is for inspection, ``qlearning_dataset`` reduces inside
    the kernel and never holds the indices."""
    _, idx = posterior_choice(preds, n_samps, MEAN, rng, return_indices=True)
    cols = (idx.to(torch.int32) & 0xffff).to(torch.int64)  # uint16 stored as int16
    return torch.gather(preds.to(torch.float32).t(), 1, cols)


# --------------------------------------------------------------------------- #
# dataset (bref:190-253)
# --------------------------------------------------------------------------- #
def qlearning_dataset(dataset: Iterable, r_model, reward_type: int, n_samples: Optional[int] = None,
                      rng=None) -> Dict[str, np.ndarray]:
    """bref:190-253; the same dict as ``custom_offline.qlearning_dataset``.

    ``r_model``: a ``PosteriorRewardNet`` or anything with ``predictions(obs_act) -> device [S, N]`` (and
    ``map_predictions(obs_act) -> device [N]`` for type 3).  One call draws for the whole dataset:
    the reference draws episode by episode from the same generator, so episode boundaries do not enter
    the stream.  As in the reference, a ``reward_type`` other than 1, 2, 3 is type 0, and type 3 draws
    nothing and leaves the generator untouched.  Fewer than two posterior networks, or an episode of
    one step, raise ``ValueError`` before any draw (the reference dies there inside numpy, its
    ``squeeze()`` having turned the row into a scalar).  Deviation: types 1 and 2 with
    ``n_samples=None`` raise ``ValueError`` where the reference has a bare ``assert``."""
    if reward_type in (1, 2) and n_samples is None:
        raise ValueError(f"reward_type {reward_type} needs n_samples")
    obs, act, nxt, dones, lengths = _co._concat_episodes(dataset)
    if min(lengths) < 2:
        raise ValueError("an episode of one step: the reference's squeeze() leaves no row to draw from")
    obs_act = np.concatenate([obs, act], axis=-1)
    if reward_type == 3:
        if not hasattr(r_model, "map_predictions"):
            _map_missing()
        rewards = r_model.map_predictions(obs_act)
    else:
        preds = r_model.predictions(obs_act)
        if preds.shape[0] < 2:
            raise ValueError("a posterior of fewer than 2 networks: a must be 1-dimensional or an integer")
        if reward_type == 1:
            rewards = posterior_choice(preds, n_samples, MEAN, rng)
        elif reward_type == 2:
            rewards = posterior_choice(preds, n_samples, MEDIAN, rng)
        else:
            rewards = posterior_choice(preds, 1, MEAN, rng)
    return {"observations": obs, "actions": act, "next_observations": nxt,
            "rewards": rewards.cpu().numpy().astype(np.float32), "terminals": dones}


# --------------------------------------------------------------------------- #
# train (bref:625-778)
# --------------------------------------------------------------------------- #
def train(config: TrainConfig, dataset=None, reward_model=None, eval_env=None, **kw):
    """bref:625-778 = ``custom_offline.train`` (same keywords: ``logger``, ``normalized_score``,
    ``seeds_per_gpu``, ``sampler``, ``device``, ``chunk``) with the posterior relabel, which runs before
    ``set_seed(train_seed)`` and so consumes numpy's global generator in whatever state it is, and the
    best model chosen by the mean evaluation return.

    ``reward_model``: a ``PosteriorRewardNet``; None reads ``config.saved_dir`` with
    ``PosteriorRewardNet.from_saved_dir``.  ``reward_type`` 3 needs its MAP weights (no ``find_map``
    here: ``NotImplementedError`` without them).

    No ``resume``: the relabel above draws from numpy's global generator before the run is seeded, so a second
    start would not relabel as the first did (``custom_offline.train(resume=True)`` is the flavour that resumes)."""
    if kw.get("resume"):
        raise NotImplementedError("custom_offline_br.train does not resume: its posterior relabel draws from numpy's "
                                  "global generator before the run is seeded")
    if reward_model is None:
        if config.reward_type == 3:
            _map_missing()
        reward_model = PosteriorRewardNet.from_saved_dir(
            config.saved_dir, config.transfer_fn, kw.get("device") or _co.D.local_device() or "cuda:0")
    if config.reward_type == 3 and getattr(reward_model, "map_set", True) is None:
        _map_missing()
    relabel = lambda ds: qlearning_dataset(ds, reward_model, config.reward_type, config.n_samples)
    return _co._train(config, dataset, eval_env, relabel, True, **kw)
