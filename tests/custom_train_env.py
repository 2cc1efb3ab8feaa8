"""Stand-ins for what ``custom_offline.train`` (cref:597-749) reads from Minari and the reward model
(test infrastructure, our own code).

``tests/golden/make_custom_train_fixture.py`` hands them to the REFERENCE's ``train()``; the GPU
tests hand fresh copies built from the same seeds to ours.  Everything is a function of the seeds.
"""
import numpy as np

from tests import fake_envs

ENV = "pen-human-v1"  # (45, 24): the pen sweeps' shape


class MinariEnv(fake_envs.FakeGymnasiumEnv):
    """A gymnasium-API environment with the spaces ``train`` reads (state / action dims, max action)."""

    def __init__(self, name=ENV):
        super().__init__(name)
        self.observation_space, self.action_space = fake_envs._Box(self.S, np.inf), fake_envs._Box(self.A, 1.0)


class MinariDataset:
    """The part of a ``minari.MinariDataset`` that cref's ``train`` uses: iteration over episodes
    and ``recover_environment()``."""

    def __init__(self, seed, lengths, name=ENV):
        self.name = name
        S, A = fake_envs.DIMS[name]
        self.episodes = fake_envs.make_episodes(seed, S, A, lengths)

    def __iter__(self):
        return iter(self.episodes)

    def recover_environment(self):
        return MinariEnv(self.name)


def reward_layers(seed, S, A, hidden=32):
    """Parameters of a one-hidden-layer Markovian reward MLP (reward_models/q_mlp.py layout:
    flax kernels [in, out])."""
    rng = np.random.default_rng(seed)
    dims = (S + A, hidden, 1)
    return [{"kernel": (rng.standard_normal((i, o)) / np.sqrt(i)).astype(np.float32),
             "bias": (0.1 * rng.standard_normal(o)).astype(np.float32)} for i, o in zip(dims[:-1], dims[1:])]


def numpy_reward(layers):
    """The stand-in of a loaded QMLP (relu hidden, no final activation) for the reference: fp32
    numpy, inputs through float32 first as a JAX model without x64 takes them."""
    def r(obs, act):
        x = np.concatenate([np.asarray(obs, np.float32), np.asarray(act, np.float32)], axis=-1)
        for i, l in enumerate(layers):
            x = x @ l["kernel"] + l["bias"]
            if i < len(layers) - 1:
                x = np.maximum(x, 0)
        return x[..., 0]
    return r
