"""sdfgpu_set_option on a fresh handle: every row of the header's table is accepted at its default, every retired name is an
unknown name, and a device build behind both still equals the exact EDT."""
import numpy as np
import pytest
import torch

import option_table as T
from oracle import oracle as O
from sdf_tools_amd import capi, synth

pytestmark = pytest.mark.gpu
SDFGPU_ERR_INVALID_ARGUMENT = -1


def _set_every_row_at_its_default(ctx):
    rows = [(n, d) for n, _, d in T.header_table() if n != "redzone"]
    assert len(rows) > 30
    for name, default in rows:
        assert (default is None) == (name == "policy_reset"), name
        ctx.set_option(name, 1 if default is None else default)


def _refused(ctx, name):
    with pytest.raises(capi.SdfGpuError) as e:
        ctx.set_option(name, 1)
    assert e.value.code == SDFGPU_ERR_INVALID_ARGUMENT
    assert name in str(e.value)


def _build_device(ctx, m):
    m_t = torch.from_numpy(m).cuda()
    assert m_t.data_ptr() % 16 == 0                  # (the vectorised pack kernel, not the generic loader)
    out = torch.empty(m.shape, dtype=torch.float32, device="cuda")
    ctx.build_device(m_t.data_ptr(), m.shape, out.data_ptr(), 1.0, False, torch.cuda.current_stream().cuda_stream)
    ext = ctx.get_extrema()
    return out.cpu().numpy(), ext


def test_defaults_accepted_retired_refused_and_builds_exact():
    """One fresh handle of its own, in this order: the table's rows, the retired names, a build and its complement."""
    ctx = capi.SdfGpu(0)
    try:
        _set_every_row_at_its_default(ctx)
        for name in T.RETIRED:
            _refused(ctx, name)
        # 40 * 32 * 32 / 16 = 2560 sixteen-byte groups against 1024 per workgroup of the pack kernel: its last workgroup is
        # partial; nz = 32 is a shape of the tuned dense tier
        m = synth.bernoulli_mask((40, 32, 32), 0.3, seed=7)
        for mask in (m, (1 - m).astype(np.uint8)):
            want, want_ext, _ = O.exact_sdf(mask, 1.0)
            sdf, ext = _build_device(ctx, mask)
            bad = np.argwhere(sdf != want)
            assert np.array_equal(sdf.view(np.uint32), want.view(np.uint32)), "%d voxels differ, first at %s" % (len(bad), bad[:4].tolist())
            assert ext == want_ext
            assert ctx.last_build_info()["dense"]
    finally:
        ctx.close()

