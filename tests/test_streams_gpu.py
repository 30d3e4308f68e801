"""The allocation rule of gpuacceleratedtracking_amd/streams.py does its job on the device: the output an operator allocates by
default puts every block start on a 16-byte boundary, so an aligned input runs the tiled / streaming kernel
(gat_last_launch_info's ``vec`` > 1).  A block stride off the rule fails no comparison of values -- the plan picks the general
kernel and only a benchmark would notice -- so this is where it is pinned."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, B, N, STRIDE = 2, 3, 1001, 1004  # every input block on a 16-byte boundary, no block length a multiple of 8


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def test_default_outputs_land_on_the_fast_path(g):
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(77)
    x = tuple(torch.from_numpy(rng.standard_normal((M, B * STRIDE)).astype(np.float32)).to(ctx.device) for _ in range(2))
    vec = lambda: ctx.last_launch_info()["vec"]  # noqa: E731
    taps = rng.standard_normal(8) + 1j * rng.standard_normal(8)

    _, d = g.filter_samples(x, taps, N, B, block_stride=STRIDE)
    assert vec() > 1 and d.block_stride == 996  # Q = 994
    for T, J in ((2, 1), (3, 2)):  # N - T + 1 = 1000 and 999 outputs a block
        w = torch.from_numpy(rng.standard_normal((J, M * T)) + 1j * rng.standard_normal((J, M * T)))
        _, d = g.spacetime_filter(x, w, T, N, B, block_stride=STRIDE)
        assert vec() > 1 and d.block_stride == 1000, (T, J)
    params = torch.tensor([[1.0, 0.0, 0.0, 1e30]] * M)
    _, d, _ = g.condition_samples(x, params, N, B, torch.int8, block_stride=STRIDE)
    assert vec() > 1 and d.block_stride == 1008

    # beams of the raw samples: the documented default is unpadded, blocks back to back
    w = torch.from_numpy(rng.standard_normal((2, M)) + 1j * rng.standard_normal((2, M)))
    y = g.beamform_samples(x, w, N, B, block_stride=STRIDE)
    assert vec() == 1 and tuple(y[0].shape) == (2, B * N)
    y = g.beamform_samples(x, w, N, B, block_stride=STRIDE, out_block_stride=STRIDE)
    assert vec() == 4 and tuple(y[0].shape) == (2, B * STRIDE)

    # the streams: one block of 1008 samples behind 8 taps, 1001 outputs in rows padded to 16 bytes
    w = torch.from_numpy(rng.standard_normal((2, M * 8)) + 1j * rng.standard_normal((2, M * 8)))  # Q = 16
    for interleaved in (False, True):
        y, d = g.filter_stream(x, taps, 1008, interleaved=interleaved)
        assert vec() > 1 and d.num_samples == 1001 and tuple((y if interleaved else y[0]).shape)[:2] == (M, 1001), interleaved
        y, d = g.spacetime_stream(x, w, 8, 1008, interleaved=interleaved)
        assert vec() > 1 and d.num_samples == 1001 and tuple((y if interleaved else y[0]).shape)[:2] == (2, 1001), interleaved
    ctx.sync()
