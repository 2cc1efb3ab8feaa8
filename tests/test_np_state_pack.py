"""Host side of the device index stream (iqlpref_amd.custom_offline.NumpyIndexStream): a numpy legacy
MT19937 state packed into the [625] uint32 words the kernel reads (key[624], pos) and back.  No GPU."""
import numpy as np
import pytest

from iqlpref_amd import custom_offline as co


@pytest.mark.parametrize("prep", ["fresh", "random3", "gauss", "pos0"])
def test_pack_unpack_round_trip(prep):
    rs = np.random.RandomState(1234)
    if prep == "random3":
        rs.random_sample(3)
    elif prep == "gauss":
        rs.standard_normal()  # leaves has_gauss = 1 and a cached value
    elif prep == "pos0":
        st = rs.get_state()
        rs.set_state((st[0], st[1], 0, 0, 0.0))
    st = rs.get_state()
    packed = co.pack_np_state(st)
    assert packed.dtype == np.uint32 and packed.shape == (co.NP_STATE_WORDS,)
    np.testing.assert_array_equal(packed[:624], st[1])
    assert int(packed[624]) == st[2]
    back = co.unpack_np_state(packed.view(np.int32), st)  # (the device buffer is int32)
    assert back[0] == "MT19937" and back[2] == st[2] and back[3] == st[3] and back[4] == st[4]
    np.testing.assert_array_equal(back[1], st[1])
    other = np.random.RandomState(0)
    other.set_state(back)
    np.testing.assert_array_equal(other.randint(0, 1000, 50), rs.randint(0, 1000, 50))


def test_pack_rejects_bad_states():
    st = np.random.RandomState(0).get_state()
    with pytest.raises(ValueError):
        co.pack_np_state(("PCG64",) + st[1:])
    with pytest.raises(ValueError):
        co.pack_np_state((st[0], st[1], 625, 0, 0.0))
    with pytest.raises(ValueError):
        co.pack_np_state((st[0], st[1][:100], 0, 0, 0.0))
