"""Stand-ins and a numpy restatement for the Bayesian-reward flavour (``custom_offline_br``, bref =
algorithms/custom_offline/iql_br.py).  Test infrastructure, our own code; everything is a function of
the seeds.

``tests/golden/make_br_fixture.py`` hands ``NumpyPosterior`` to the REFERENCE's ``posterior_sampler`` /
``qlearning_dataset`` / ``train``; the tests hand the same weights (or the recorded predictions) to ours.
"""
import numpy as np

from tests import custom_train_env as cte

HIDDEN = 16


def posterior_layers(seed, n_post, S, A, hidden=HIDDEN):
    """``n_post`` weight sets of a one-hidden-layer reward MLP, each as the BNN sampler stores one:
    [W0, b0, W1, b1] with W [in, out].  Set k is ``cte.reward_layers(seed + k)``."""
    sets = []
    for k in range(n_post):
        layers = cte.reward_layers(seed + k, S, A, hidden)
        sets.append([a for l in layers for a in (l["kernel"], l["bias"])])
    return sets


def numpy_forward(w, x):
    """fp32 numpy forward of one weight set (relu hidden), inputs through float32 first."""
    x = np.asarray(x, np.float32)
    n_layers = len(w) // 2
    for i in range(n_layers):
        x = x @ w[2 * i] + w[2 * i + 1]
        if i < n_layers - 1:
            x = np.maximum(x, 0)
    return x


class NumpyPosterior:
    """What bref reads of a ``PrefNet``: ``predict(X, True)`` -> (None, None, [S, T, 1]) posterior
    predictions; ``predict(X, use_map=True)`` -> (None, None, [1, T, 1]) from the MAP weight set.  (The
    name of the second positional parameter lives in the absent optbnn submodule; bref only ever passes
    True there, so it is accepted and ignored.)"""

    def __init__(self, sets, map_set=None):
        self.sets, self.map_set = sets, map_set
        self.sampled_weights = None

    def _load_all_sampled_weights(self):
        return iter(())

    def predict(self, X, _individual=True, use_map=False):
        if use_map:
            return None, None, numpy_forward(self.map_set, X)[None]
        return None, None, np.stack([numpy_forward(w, X) for w in self.sets])


class RecordedPosterior:
    """``predictions`` / ``map_predictions`` from recorded host matrices, uploaded: the reward model of a
    test that wants the reference's predictions to the bit."""

    def __init__(self, preds, map_preds=None, device="cuda:0"):
        self.preds, self.map_preds, self.device = preds, map_preds, device
        self.map_set = None if map_preds is None else ()

    def predictions(self, obs_act):
        import torch
        assert len(obs_act) == self.preds.shape[1]
        return torch.from_numpy(np.ascontiguousarray(self.preds, np.float32)).to(self.device)

    def map_predictions(self, obs_act):
        import torch
        return torch.from_numpy(np.ascontiguousarray(self.map_preds, np.float32)).to(self.device)


def obs_act_of(dataset):
    """[N, S + A] of a fake Minari dataset, episode after episode (bref:197-199)."""
    return np.concatenate([np.concatenate([e.observations[:-1], e.actions], axis=-1) for e in dataset])


def predictions_of(sets, dataset):
    """[S, N] stand-in predictions as bref asks for them: one ``predict`` per episode (a BLAS matmul
    rounds a row differently in matrices of different height, so the whole dataset in one forward
    differs in the last bit here and there)."""
    return np.concatenate([np.stack([numpy_forward(w, np.concatenate([e.observations[:-1], e.actions], axis=-1))[:, 0]
                                     for w in sets]) for e in dataset], axis=1)


# --------------------------------------------------------------------------- #
# numpy restatement of bref:179-253 as ONE randint stream
# --------------------------------------------------------------------------- #
def choice_indices(S, N, n_samps, rng=None):
    """The claim under test: N consecutive ``np.random.choice(row_of_length_S, n_samps)`` draw
    ``randint(0, S, size=(N, n_samps))``."""
    return (np.random if rng is None else rng).randint(0, S, size=(N, n_samps))


def posterior_sampler(preds_sn, n_samps, rng=None):
    """[S, N] -> ([N, n_samps] samples, [N, n_samps] indices)."""
    S, N = preds_sn.shape
    idx = choice_indices(S, N, n_samps, rng)
    # (C-contiguous rows, as the reference's np.stack of per-row draws: mean(1) then sums in its order)
    return np.ascontiguousarray(np.take_along_axis(preds_sn.T, idx, axis=1)), idx


def relabel(preds_sn, map_preds, reward_type, n_samples=None, rng=None):
    """The rewards of bref:190-253 from the [S, N] predictions of the whole dataset."""
    if reward_type == 3:
        return np.asarray(map_preds)
    if reward_type == 1:
        return posterior_sampler(preds_sn, n_samples, rng)[0].mean(1)
    if reward_type == 2:
        return np.median(posterior_sampler(preds_sn, n_samples, rng)[0], axis=1)
    return posterior_sampler(preds_sn, 1, rng)[0][:, 0]
