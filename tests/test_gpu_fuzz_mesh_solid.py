"""GPU: a few seconds of tools/fuzz_mesh_solid.py: random closed meshes (randomly posed icosahedra, tori and boxes, randomly subdivided,
with random flips and as soups) on random small grids and origins, the device form against the numpy restatement."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_a_few_seconds_of_random_closed_meshes(gpu, capsys):
    import fuzz_mesh_solid
    scenes, filled, inside = fuzz_mesh_solid.run(3.0, 1, least=40)
    print("%d scenes, %d filled cells, %d of them by parity alone" % (scenes, filled, inside))
    assert scenes >= 40 and inside > 1000


def test_a_dozen_random_tall_scenes(gpu, capsys):
    """mesh_solid_cases.random_tall_scene: narrow grids whose nz lies about one word, two words and 64 words (the chunk carry with
    random toggles below it), through the same differential run"""
    import fuzz_mesh_solid
    import mesh_solid_cases as SC
    grids = [SC.random_tall_scene(seed)[5] for seed in range(12)]
    assert sum(g[2] > 2048 for g in grids) >= 3 and any(g[2] <= 64 for g in grids) and any(64 < g[2] <= 70 for g in grids)
    scenes, filled, inside = fuzz_mesh_solid.run(0.0, 2, generator=(SC.random_tall_scene(seed) for seed in range(12)))
    print("%d tall scenes, %d filled cells, %d of them by parity alone" % (scenes, filled, inside))
    assert scenes == 12 and inside > 1000
