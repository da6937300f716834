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
