"""Environments only: the normalising wrapper of the evaluation loops, a list of wrapped environments stepped
by lane number, and the program of an environment worker process of ``posthoc.evaluate_many``.

This file imports nothing of the package and nothing beyond the standard library, and ``posthoc`` starts a
worker by running it BY PATH in a fresh interpreter (``python .../_env_worker.py``): a worker never executes
``iqlpref_amd/__init__`` and so never imports torch, the ctypes binding or the trainer modules.  It holds the
environments ``make_env`` builds and whatever their own modules import.

Protocol (``multiprocessing.connection``, authenticated with a key read from standard input): the first
message is ``(sys_path, pickled make_env, n, state_mean, state_std)``; then ``(op, items)`` with op ``seed`` /
``reset`` / ``step`` is answered with ``("ok", Lanes.op(items))`` or ``("error", traceback text)``, and
``("close", None)`` ends the process."""
import sys


class NormalizedEnv:
    """What the reference builds from gym.wrappers.TransformObservation / TransformReward
    (ref:140-161), without importing gym: observations are z-scored with the dataset
    statistics on the way out of reset() / step(), rewards are scaled.  Everything else is the
    wrapped environment's."""

    def __init__(self, env, state_mean, state_std, reward_scale):
        self.env = env
        self._mean, self._std, self._scale = state_mean, state_std, reward_scale

    def __getattr__(self, name):
        return getattr(self.env, name)

    def _obs(self, obs):
        return (obs - self._mean) / self._std  # the epsilon is already part of state_std

    def reset(self, **kw):
        out = self.env.reset(**kw)
        return (self._obs(out[0]),) + tuple(out[1:]) if isinstance(out, tuple) else self._obs(out)

    def step(self, action):
        obs, reward, *rest = self.env.step(action)
        return (self._obs(obs), reward * self._scale if self._scale != 1.0 else reward, *rest)


def wrap_env(env, state_mean=0.0, state_std=1.0, reward_scale: float = 1.0):
    """ref:140-161: normalised observations (and scaled rewards) around ``env``."""
    return NormalizedEnv(env, state_mean, state_std, reward_scale)


def unpack_step(out):
    """(obs, reward, done) of a gymnasium (terminated, truncated) or a gym < 0.26 (done) step."""
    if len(out) == 5:
        obs, reward, terminated, truncated, _ = out
        return obs, reward, bool(terminated or truncated)
    obs, reward, done, _ = out
    return obs, reward, bool(done)


class Lanes:
    """``n`` wrapped environments of this process.  seed(items): [(lane, seed)] (gym < 0.26);
    reset(items): [(lane, seed or None)] -> observations; step(items): [(lane, action)] -> [(obs, reward, done)]."""

    def __init__(self, make_env, n, state_mean, state_std):
        self.envs = [wrap_env(make_env(), state_mean=state_mean, state_std=state_std) for _ in range(n)]

    def seed(self, items):
        for lane, s in items:
            self.envs[lane].seed(s)

    def reset(self, items):
        out = []
        for lane, s in items:
            o = self.envs[lane].reset() if s is None else self.envs[lane].reset(seed=s)
            out.append(o[0] if isinstance(o, tuple) else o)
        return out

    def step(self, items):
        return [unpack_step(self.envs[lane].step(a)) for lane, a in items]

    def close(self):
        for e in self.envs:
            close = getattr(e, "close", None)
            if close is not None:
                close()


def main(address):
    import pickle
    import traceback
    from multiprocessing.connection import Client
    authkey = bytes.fromhex(sys.stdin.readline().strip())
    conn = Client(address, authkey=authkey)
    lanes = None
    try:
        try:
            path, make_env, n, state_mean, state_std = conn.recv()
            sys.path[:] = path
            lanes = Lanes(pickle.loads(make_env), n, state_mean, state_std)
            conn.send(("ok", None))
        except Exception:
            conn.send(("error", traceback.format_exc()))
            return 1
        while True:
            op, items = conn.recv()
            if op == "close":
                return 0
            try:
                conn.send(("ok", getattr(lanes, op)(items)))
            except Exception:
                conn.send(("error", traceback.format_exc()))
    except EOFError:  # the parent has gone
        return 1
    finally:
        if lanes is not None:
            lanes.close()
        conn.close()


if __name__ == "__main__":
    del sys.path[0]  # this file's directory: the package's modules are not top-level modules
    sys.exit(main(sys.argv[1]))
