"""Stand-in for what ``minari_iql.train`` and ``minari_bc.train`` read from Minari (test infrastructure, our own
code): a dataset whose episodes carry ``id`` and ``rewards`` and that has ``iterate_episodes(episode_indices=)``.

``tests/golden/make_minari_fixture.py`` hands it to the REFERENCE's two ``train()`` functions; the tests hand fresh
copies built from the same seeds to ours.  Everything is a function of the arguments.

The rewards are built so that the any-percent selection meets its two awkward cases at once: episode e pays
``LEVELS[e]`` plus noise per step, which orders the discounted returns as 4 > 2 > 1 = 3 > 6 > 0 > 5 -- episodes 1
and 3 have the same length and the SAME rewards, so they tie exactly -- and with 7 episodes ``top_fraction =
0.45`` asks for 3.15 of them: three are kept, and the tie sits on the boundary (a stable sort keeps 1, drops 3).
"""
import numpy as np

from tests import custom_train_env as cte
from tests import fake_envs

LENGTHS = (40, 55, 33, 55, 47, 52, 38)
LEVELS = (0.2, 0.5, 0.9, 0.5, 0.7, 0.1, 0.3)
TIE = (1, 3)  # episode 3 repeats episode 1's rewards
TOP_FRACTION = 0.45


class Episode:
    """The fields of a minari EpisodeData the two programs read."""

    def __init__(self, id, observations, actions, rewards, terminations):
        self.id, self.observations, self.actions = id, observations, actions
        self.rewards, self.terminations = rewards, terminations


class MinariDataset:
    def __init__(self, seed, lengths=LENGTHS, levels=LEVELS, name=cte.ENV, reward_dtype=np.float64):
        self.name = name
        S, A = fake_envs.DIMS[name]
        rng = np.random.default_rng(seed)
        self.episodes = []
        for e, (L, level) in enumerate(zip(lengths, levels)):
            term = np.zeros(L, dtype=bool)
            term[-1] = rng.uniform() < 0.5
            rewards = (level + 0.1 * rng.standard_normal(L)).astype(reward_dtype)
            self.episodes.append(Episode(e, rng.standard_normal((L + 1, S)), rng.uniform(-1, 1, (L, A)), rewards, term))
        a, b = TIE
        if len(self.episodes) > b and lengths[a] == lengths[b]:
            self.episodes[b].rewards = self.episodes[a].rewards.copy()

    def __iter__(self):
        return iter(self.episodes)

    def __len__(self):
        return len(self.episodes)

    def iterate_episodes(self, episode_indices=None):
        ids = range(len(self.episodes)) if episode_indices is None else episode_indices
        return (self.episodes[i] for i in ids)

    def recover_environment(self):
        return cte.MinariEnv(self.name)
