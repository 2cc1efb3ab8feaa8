"""custom_offline.train(): the services it cannot find are named before any GPU work.  No GPU."""
import pytest

from iqlpref_amd import custom_offline as co
from tests import custom_train_env as cte


def _config():
    return co.TrainConfig(update_steps=10, eval_every=5)


def test_without_reward_model_names_orbax():
    with pytest.raises((ImportError, NotImplementedError), match="[Oo]rbax"):
        co.train(_config(), cte.MinariDataset(11, (20, 30)), None, device="cuda:0")


def test_without_dataset_names_minari(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "minari", None)  # (import minari raises ImportError)
    with pytest.raises(ImportError, match="minari"):
        co.train(_config(), None, object(), device="cuda:0")


def test_bad_arguments():
    ds = cte.MinariDataset(11, (20, 30))
    with pytest.raises(ValueError):
        co.train(_config(), ds, object(), sampler="gpu", device="cuda:0")
    with pytest.raises(ValueError):
        co.train(_config(), ds, object(), seeds_per_gpu=17, device="cuda:0")
    with pytest.raises(ValueError, match="eval_env"):
        co.train(_config(), list(ds), object(), device="cuda:0")
