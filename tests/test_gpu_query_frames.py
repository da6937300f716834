"""sdfgpu_query_points and sdfgpu_query_points_device in general 3-D frames on the MI355X, against the exact judge of
tests/frame_judge.py: every frame of frames() (all nine rotation entries nonzero, turns about x and about y, a cyclic permutation
and its inverse, beside the identity and translation controls), edge gradients on and off, a finite and an infinite oob_value.
tests/test_frame_judge_cpu.py pins the judge, shows that it rejects transposed and exchanged matrices in these frames, and
asserts on the same points that none of the uniform ones is ambiguous."""
import math

import numpy as np
import pytest
import torch

import analysis_scenes as A
import frame_judge as J
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu
FRAMES = sorted(J.frames())
_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    c = capi.SdfGpu(0)
    yield c
    c.close()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def _case(ctx, frame, shape, res):
    """the field (built by the library, once per shape), the points and the judge's exact part, once per (frame, shape)"""
    if shape not in _CACHE:
        sdf, _ = ctx.build(J.case_mask(shape), res)
        assert np.isfinite(sdf).all()                              # both classes: no corner is infinite
        _CACHE[shape] = (sdf, torch.from_numpy(sdf).cuda())
    if (frame, shape) not in _CACHE:
        sdf = _CACHE[shape][0]
        origin = J.frames()[frame]
        w2g, rot = J.transforms(origin)
        pts, parts = J.case_points(shape, res, origin, J.case_seed(frame, shape))
        _CACHE[(frame, shape)] = (w2g, rot, pts, parts, J.Exact(sdf, res, w2g, rot, pts))
    return _CACHE[shape] + _CACHE[(frame, shape)]


@pytest.mark.parametrize("shape, res", J.FIELDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_both_forms_against_the_exact_judge(ctx, frame, shape, res):
    """The host-points form is judged; the device form is bit-equal to it (the documented claim), so the same verdict holds."""
    sdf, d_sdf, w2g, rot, pts, parts, exact = _case(ctx, frame, shape, res)
    n = len(pts)
    amb = exact.ambiguous()
    assert amb[parts["uniform"]].mean() <= J.AMBIGUITY_CAP
    assert amb[parts["lattice"]].sum() >= 32                       # the accept-either arm runs
    d_pts = torch.from_numpy(pts).cuda()
    for edge in (False, True):
        judged = J.judge(sdf, res, w2g, rot, pts, edge, exact)
        for oob in (math.inf, 7.5):
            dist, grad, flags = ctx.query_points(d_sdf.data_ptr(), shape, res, pts, world_to_grid=w2g, rotation=rot, oob_value=oob,
                                                 enable_edge_gradients=edge)
            assert dist.shape == (n,) and grad.shape == (n, 3) and flags.shape == (n,)
            dd = torch.full((n,), -77.0, dtype=torch.float64, device="cuda")
            dg = torch.full((n, 3), -77.0, dtype=torch.float64, device="cuda")
            df = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
            ctx.query_points_device(d_sdf.data_ptr(), shape, res, d_pts.data_ptr(), n, dd.data_ptr(), dg.data_ptr(), df.data_ptr(),
                                    w2g, rot, oob, edge, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert _same(dd.cpu().numpy(), dist) and _same(dg.cpu().numpy(), grad) and _same(df.cpu().numpy(), flags)
            bad = parts["bad"]                                     # NaN and inf rows: outside
            assert (flags[bad] == 0).all() and (dist[bad] == oob).all() and np.isnan(grad[bad]).all()
            got = judged.check(dist, grad, flags, oob)
            assert 0 < got["inside"] < n and got["unjudged"] == 0
            assert got["inside"] == int((flags & 1).sum())
            print("query_points %s %s edge %d oob %s: inside %d ambiguous %d, worst |error| / tolerance: distance %.4f gradient %.4f"
                  % (frame, shape, edge, oob, got["inside"], got["ambiguous"], got["distance"], got["gradient"]))
    if frame in ("identity", "translation"):                       # the controls: bit-equal to the restatement
        with np.errstate(invalid="ignore"):
            g = pts - J.frames()[frame][:3, 3]
        wd, wg, wf = A.query_points(sdf, res, g, 7.5, True)
        ok = np.isfinite(pts).all(axis=1)
        assert np.array_equal(flags, wf) and _same(dist[ok], wd[ok]) and _same(grad[ok], wg[ok])
