"""The scenes of tests/tile_lists.py do what they are for — asserted from the oracle alone, before any GPU is asked
(tests/test_gpu_tile_first_edges.py repeats these checks at the top of every test that renders a scene)."""
import numpy as np
import pytest

from tests import tile_lists as TL

SCREENS = [TL.ONE_CLASS_SCREEN, TL.TWO_CLASS_SCREEN]


def test_screens_are_on_the_class_boundary():
    tiles = [-(-w // 16) * -(-h // 16) for w, h in SCREENS]
    assert tiles[0] == 4200 and 4200 < tiles[1] < 6144  # one launch for every tile | two classes, short class 8
    assert tiles[1] == 4260
    assert all(TL.tile_id_low_bits(t) == 6 for t in tiles) and TL.tile_id_low_bits(256) == 8 and TL.tile_id_low_bits(65536) == 8


@pytest.mark.parametrize("w,h", SCREENS)
@pytest.mark.parametrize("name", ["by_length", "by_passes"])
def test_scene_holds_the_requested_lists(name, w, h):
    sc = TL.build(name, w, h)
    total = TL.check_scene(sc)
    table = sc["table"]
    if name == "by_length":
        assert table[:, 1].tolist() == TL.BY_LENGTH and len(TL.BY_LENGTH) == 34
    else:
        assert sorted(set(table[:, 1].tolist())) == sorted(TL.BY_PASSES_LENGTHS)
        for length in TL.BY_PASSES_LENGTHS:
            assert table[table[:, 1] == length, 2].tolist() == [0, 1, 2, 3, 4]
    assert total == sc["ref"]["counts"].sum()
    # the lists' members lie all over the index range (a pile is not one run of splat indices)
    t = int(table[np.argmax(table[:, 1]), 0])
    lst = sc["ref"]["indices"][sc["ref"]["offsets"][t]:][:int(sc["ref"]["counts"][t])]
    assert lst.max() - lst.min() > sc["props"].shape[0] // 2


def test_check_scene_notices_a_wrong_scene():
    """The check is not vacuous: a pile that loses a member, and a stray splat in an aligned run, both fail it."""
    sc = dict(TL.build("by_length", *TL.TWO_CLASS_SCREEN))
    table = sc["table"].copy()
    table[5, 1] += 1
    with pytest.raises(AssertionError):
        TL.check_scene(dict(sc, table=table))
    ref = dict(sc["ref"])
    counts = ref["counts"].copy()
    t4096 = int(sc["table"][sc["table"][:, 1] == 4096, 0][0])
    stray = (t4096 + 64) % counts.size  # same low digit
    assert counts[stray] == 0
    counts[stray] = 1
    ref["counts"] = counts
    with pytest.raises(AssertionError):
        TL.check_scene(dict(sc, ref=ref))


@pytest.mark.parametrize("r", [1, 2, 3])
def test_ragged_tail_scenes(r):
    TL.check_ragged_tail(TL.ragged_tail(r), r)


@pytest.mark.parametrize("kind", ["block", "giant"])
def test_multi_round_scenes(kind):
    TL.check_multi_round(TL.multi_round(kind), kind)
