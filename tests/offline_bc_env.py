"""Stand-ins for what ``offline_bc.train`` (algorithms/offline/any_percent_bc.py, "dbc") reads from gym and d4rl
(test infrastructure, our own code): a gym < 0.26 environment with ``seed``, ``get_normalized_score`` and
``action_space.high``, a D4RL-style transition dataset, and the small selection cases.

``tests/golden/make_offline_bc_fixture.py`` hands them to the REFERENCE's ``train()`` and
``keep_best_trajectories``; the tests hand fresh copies built from the same seeds to ours.  Everything is a
function of the arguments.

The training dataset has one run of 1030 rows without a terminal, so the cut at 1000 rows -- the only cut dbc's
``train()`` ever applies -- makes a 1000-row and a 30-row trajectory of it, and a trailing run without a terminal
that is dropped.  Trajectory e pays ``LEVELS[e]`` plus noise per row: all discounted returns are distinct.
"""
import numpy as np

from tests import fake_envs

ENV = "halfcheetah-medium-v2"  # (17, 6)
LENGTHS = (40, 55, 1030, 33, 47, 60, 52, 38, 25)  # the last run has no terminal: dropped
LEVELS = (0.2, 0.5, 0.3, 0.9, 0.7, 0.1, 0.35, 0.6, 5.0)  # (the 1000-row piece has the greatest return)
FRAC = 0.45  # of 9 complete trajectories (the 1030 rows are two): int(4.05) = 4 are kept
SCORE_RANGE = (-1.5, 6.5)  # get_normalized_score(x) = (x - lo) / (hi - lo)


class OfflineBCEnv(fake_envs.FakeGymEnv):
    """``fake_envs.FakeGymEnv`` with d4rl's ``get_normalized_score``."""

    def __init__(self, name=ENV):
        super().__init__(name)

    def get_normalized_score(self, score):
        lo, hi = SCORE_RANGE
        return (score - lo) / (hi - lo)


def make_dataset(seed, reward_dtype=np.float32, name=ENV):
    """What ``d4rl.qlearning_dataset`` returns, synthetic: float32 observations / actions / next observations,
    rewards in ``reward_dtype``, boolean terminals."""
    S, A = fake_envs.DIMS[name]
    rng = np.random.default_rng(seed)
    obs, nxt, act, rew, term = [], [], [], [], []
    for e, (L, level) in enumerate(zip(LENGTHS, LEVELS)):
        o = rng.standard_normal((L + 1, S)).astype(np.float32)
        obs.append(o[:-1]), nxt.append(o[1:])
        act.append(rng.uniform(-1, 1, (L, A)).astype(np.float32))
        rew.append((level + 0.1 * rng.standard_normal(L)).astype(reward_dtype))
        t = np.zeros(L, dtype=bool)
        t[-1] = e < len(LENGTHS) - 1
        term.append(t)
    return {"observations": np.concatenate(obs), "actions": np.concatenate(act),
            "next_observations": np.concatenate(nxt), "rewards": np.concatenate(rew), "terminals": np.concatenate(term)}


# --------------------------------------------------------------------------- #
# selection cases: name -> (n, max_len, terminal rows, fractions, ordered)
# --------------------------------------------------------------------------- #
TINY = 1e-9  # a fraction at which max(1, int(frac * n_traj)) is the 1
CASES = {
    "n1_term": (1, 1000, (0,), (1.0,), True),                      # one row, one trajectory
    "n1_open": (1, 1000, (), (1.0,), True),                        # no complete trajectory at all
    "single": (20, 1000, (19,), (TINY, 1.0), True),                # one trajectory
    "m1_n50": (50, 1, (3, 4, 20, 49), (TINY, 0.3, 1.0), True),     # every row is a trajectory
    # cuts at 7 rows: the terminal at 6 falls on a cut, 9 opens a new phase, 16 = 9 + 7 falls on a cut again,
    # 17 is a one-row trajectory, then cuts alone; the last 4 rows are dropped
    "m7_n50": (50, 7, (6, 9, 16, 17), (TINY, 0.5, 1.0), True),
    "term_at_cut": (30, 10, (9, 19), (0.5, 1.0), True),             # terminals exactly where the cut falls
    "trailing": (40, 1000, (10, 25), (0.5, 1.0), True),            # the 14 rows behind row 25 are dropped
    "chunks": (3001, 1000, (1500, 2800), (TINY, 0.5, 1.0), True),  # crosses the scan's 1024-row chunks
    "ties": (60, 1000, tuple(range(5, 60, 6)), (0.25, 1.0), False),  # all returns zero: order is the host's
}
ACTION_WIDTH = 3


def selection_case(name, reward_dtype=np.float32):
    """The dataset of one case.  Observations [n, 1] hold the row number and next observations the row number
    + 0.5 (exact in float32): the selected observations ARE the reference's ``order``."""
    n, max_len, term_rows, fracs, ordered = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    ids = np.arange(n, dtype=np.float32)[:, None]
    term = np.zeros(n, dtype=bool)
    term[list(term_rows)] = True
    rew = rng.standard_normal(n).astype(reward_dtype) if ordered else np.zeros(n, reward_dtype)
    return {"observations": ids, "actions": rng.uniform(-1, 1, (n, ACTION_WIDTH)).astype(np.float32),
            "next_observations": ids + np.float32(0.5), "rewards": rew, "terminals": term}
