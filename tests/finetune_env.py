"""Stand-ins for the online fine-tuning runs (test infrastructure, our own code).

``FinetuneEnv`` is a small deterministic gym < 0.26 environment (S = 5, A = 3, episodes of at most 7
steps, some ending earlier in a true termination) that the REFERENCE's ``finetune/iql.py:train`` drives
when ``tests/golden/make_finetune_fixture.py`` records a run.  ``RecordingEnv`` writes down everything it
hands out; ``ReplayEnv`` hands the same things out again in the same order, whatever actions it is given,
so that a second run of the loop cannot fork from the first through rounding in its actor -- it keeps the
actions it was given for the comparison.
"""
import zlib

import numpy as np

S, A, MAX_EPISODE_STEPS = 5, 3, 7


class _Box:
    def __init__(self, n, high):
        self.shape, self.high, self.low = (n,), np.full(n, high), np.full(n, -high)

    def seed(self, seed):
        self.seeded = seed


class FinetuneEnv:
    """state' = 0.8 state + 0.2 tanh(M a) + noise.  The horizon of an episode is drawn at reset from 3..7:
    one that ends before step 7 is a true termination, one of 7 steps a timeout.  Names with "antmaze" are
    goal environments: sparse reward 1 on the last step of a successful episode and ``goal_achieved`` in
    ``info``; the others pay a smooth function of action and state and report nothing."""

    def __init__(self, name):
        self.name = name
        self.goal = "antmaze" in name
        self._max_episode_steps = MAX_EPISODE_STEPS
        self.observation_space, self.action_space = _Box(S, np.inf), _Box(A, 1.0)
        self.M = np.random.default_rng(zlib.crc32(name.encode())).standard_normal((S, A)) / np.sqrt(A)
        self.rng = np.random.default_rng(0)

    def seed(self, seed):
        self.rng = np.random.default_rng(int(seed))

    def reset(self):
        self.t = 0
        self.horizon = int(self.rng.integers(3, MAX_EPISODE_STEPS + 1))
        self.success = bool(self.rng.uniform() < 0.5)
        self.state = self.rng.standard_normal(S)
        return self.state.copy()

    def step(self, action):
        a = np.asarray(action, dtype=np.float64).reshape(A)
        self.t += 1
        self.state = 0.8 * self.state + 0.2 * np.tanh(self.M @ a) + 0.05 * self.rng.standard_normal(S)
        done = self.t >= self.horizon
        if self.goal:
            hit = bool(done and self.success)
            return self.state.copy(), 1.0 if hit else 0.0, done, {"goal_achieved": hit}
        return self.state.copy(), float(0.1 * a.sum() + 0.05 * self.state[0] + 0.02), done, {}

    def get_normalized_score(self, score):
        return (score + 1.0) / 4.0


def make_dataset(name, n, seed):
    """A d4rl-style transition dict of ``n`` rows rolled out of ``FinetuneEnv(name)`` with random actions."""
    env, rng = FinetuneEnv(name), np.random.default_rng(seed)
    env.seed(seed)
    out = {k: [] for k in ("observations", "actions", "rewards", "next_observations", "terminals")}
    state, steps = env.reset(), 0
    for _ in range(n):
        a = rng.uniform(-1, 1, A)
        nxt, r, done, _ = env.step(a)
        steps += 1
        out["observations"].append(state), out["actions"].append(a), out["rewards"].append(r)
        out["next_observations"].append(nxt), out["terminals"].append(done and steps < MAX_EPISODE_STEPS)
        state = nxt
        if done:
            state, steps = env.reset(), 0
    return {"observations": np.asarray(out["observations"], np.float32), "actions": np.asarray(out["actions"], np.float32),
            "rewards": np.asarray(out["rewards"], np.float32),
            "next_observations": np.asarray(out["next_observations"], np.float32),
            "terminals": np.asarray(out["terminals"], np.float32)}


class RecordingEnv:
    """``env`` with a tape: one entry per ``reset`` / ``step`` (what came back) and the actions given."""

    def __init__(self, env):
        self.env = env
        self.kind, self.obs, self.reward, self.done, self.goal, self.actions, self.seeds = [], [], [], [], [], [], []

    def __getattr__(self, name):
        return getattr(self.env, name)

    def seed(self, seed):
        self.seeds.append(int(seed))
        self.env.seed(seed)

    def reset(self):
        obs = self.env.reset()
        self.kind.append(0), self.obs.append(obs.copy()), self.reward.append(0.0), self.done.append(False)
        self.goal.append(-1)
        return obs

    def step(self, action):
        self.actions.append(np.asarray(action, np.float64).copy())
        obs, r, done, info = self.env.step(action)
        self.kind.append(1), self.obs.append(obs.copy()), self.reward.append(float(r)), self.done.append(bool(done))
        self.goal.append(int(info["goal_achieved"]) if "goal_achieved" in info else -1)
        return obs, r, done, info

    def tape(self, prefix):
        return {f"{prefix}/kind": np.asarray(self.kind, np.int8), f"{prefix}/obs": np.asarray(self.obs, np.float64),
                f"{prefix}/reward": np.asarray(self.reward, np.float64), f"{prefix}/done": np.asarray(self.done, bool),
                f"{prefix}/goal": np.asarray(self.goal, np.int8),
                f"{prefix}/actions": np.asarray(self.actions, np.float64).reshape(-1, A),
                f"{prefix}/seeds": np.asarray(self.seeds, np.int64)}


class ReplayEnv:
    """Hands out a ``RecordingEnv`` tape again; a call of the other kind than the tape's next entry is an
    error (the loop under test took another path than the recorded one)."""

    def __init__(self, name, tape, prefix):
        self.name = name
        self._max_episode_steps = MAX_EPISODE_STEPS
        self.observation_space, self.action_space = _Box(S, np.inf), _Box(A, 1.0)
        self._t = {k[len(prefix) + 1:]: v for k, v in tape.items() if k.startswith(prefix + "/")}
        self._i = 0
        self.actions, self.seeds = [], []

    def seed(self, seed):
        self.seeds.append(int(seed))

    def _next(self, kind):
        i = self._i
        if i >= len(self._t["kind"]) or self._t["kind"][i] != kind:
            raise AssertionError(f"tape entry {i}: the loop asks for a {'step' if kind else 'reset'} the recording "
                                 "does not have there")
        self._i += 1
        return i

    def reset(self):
        return self._t["obs"][self._next(0)].copy()

    def step(self, action):
        self.actions.append(np.asarray(action, np.float64).copy())
        i = self._next(1)
        g = int(self._t["goal"][i])
        return (self._t["obs"][i].copy(), float(self._t["reward"][i]), bool(self._t["done"][i]),
                {"goal_achieved": bool(g)} if g >= 0 else {})

    def exhausted(self):
        return self._i == len(self._t["kind"])

    def get_normalized_score(self, score):
        return (score + 1.0) / 4.0
