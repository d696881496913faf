"""The scenes of tests/front_boundary_scenes.py sit on the boundaries they are built for: every condition asserted on the CPU oracle alone
(no GPU).  tests/test_gpu_front_boundaries.py asserts them again before it compares the HIP path with the oracle on these scenes."""
import numpy as np
import pytest

import front_boundary_scenes as fb


def test_pass_counts_at_the_edges():
    """1 pass up to 256 tiles, 2 up to 65 536, 3 above (gwbp_dev.h sort_passes); fin = passes & 1 is the buffer the lists end in."""
    assert [fb.sort_passes(n) for n in (1, 2, 256, 257, 65536, 65537, 80000, 1 << 24)] == [1, 1, 1, 2, 2, 3, 3, 3]
    assert {fb.n_tiles(*fb.TILE_SCENES[k][:2]): p for k, p in fb.TILE_PASSES.items()} == {1: 1, 256: 1, 272: 2, 65536: 2, 80000: 3}


@pytest.mark.parametrize("name", list(fb.TILE_SCENES))
def test_tile_count_scene_sits_on_its_pass_count(orc, name):
    facts = fb.check_tile_scene(name)
    print(name, facts)
    assert fb.TILE_SCENES[name][2] <= 2000  # (a few hundred to 2000 Gaussians)


@pytest.mark.parametrize("n,image,n_depths", fb.TIE_CASES, ids=fb.TIE_IDS)
def test_tie_scene_has_ties_in_every_block(orc, n, image, n_depths):
    facts = fb.check_tie_scene(n, image, n_depths)
    print(n, image, facts)
    # the oracle itself keeps the contract the GPU is compared against: inside every tile list (depth, index) ascends, and with
    # at most three depths nearly every neighbour is a tie resolved by index
    sc = fb.tie_scene(n, image, n_depths)
    proj, bins = fb.front(sc)
    flat, offs = bins["flatten_ids"].astype(np.int64), bins["tile_offsets"]
    key = proj["depths"].view(np.uint32)[flat].astype(np.int64) * (1 << 32) + flat
    inner = np.ones(len(flat), bool)
    inner[offs[:-1][offs[:-1] < len(flat)]] = False  # the first entry of a list has no predecessor in it
    assert (np.diff(key)[inner[1:]] > 0).all()
    assert (proj["radii"][flat] > 0).all()


def test_tie_cases_cover_both_sides_of_every_depth_sort_path():
    counts = {n for n, image, _ in fb.TIE_CASES if image == "small"}
    for edge in fb.SMALL_SORT:
        assert {edge, edge + 1} <= counts
    assert {1, 16384, 16385, 20481} <= counts  # one key; a full last block, one key in the last block, a partial one


@pytest.mark.parametrize("target", fb.BLOCK_TARGETS)
def test_block_scene_hits_its_intersection_count(orc, target):
    print(target, fb.check_block_scene(target))


def test_block_targets_surround_a_block_boundary():
    assert {fb.SORT_BLOCK - 1, fb.SORT_BLOCK, fb.SORT_BLOCK + 1, 2 * fb.SORT_BLOCK, 1} <= set(fb.BLOCK_TARGETS)
    assert fb.BIG_TARGET % fb.SORT_BLOCK == 0
