"""gpuacceleratedtracking_amd/streams.py without a device: the allocation rule of a stream output against the rule written out
here, the one window check at its edge, the overlap-save geometry against its two formulas, and a descriptor of ``alloc_stream``
accepted by the library's host twin."""
import numpy as np
import pytest
import torch

PLANAR, CF32, I16, I8 = 0, 1, 2, 3
# (dtype, planar) -> layout, samples per 16 bytes: 4 planar float32, 2 ComplexF32, 4 int16 pairs, 8 int8 pairs
LAYOUTS = {(torch.float32, True): (PLANAR, 4), (torch.float32, False): (CF32, 2), (torch.int16, False): (I16, 4), (torch.int8, False): (I8, 8)}


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.mark.parametrize("dtype,planar", list(LAYOUTS))
def test_alloc_stream_pads_every_block_start_to_16_bytes(g, dtype, planar):
    layout, vs = LAYOUTS[(dtype, planar)]
    for N in range(1, 18):
        for nb in (1, 3):
            for M in (1, 3):
                out, d = g.streams.alloc_stream(M, N, nb, "cpu", dtype, planar)
                stride = -(-N // vs) * vs
                assert d.block_stride == stride and d.ant_stride == nb * stride, (N, nb, M)
                assert (d.num_samples, d.num_ants, d.layout, d.chan_stride) == (N, M, layout, 0)
                first = out[0] if planar else out
                assert d.re == first.data_ptr() and d.re % 16 == 0
                assert d.im == (out[1].data_ptr() if planar else None)
                for t in (out if planar else (out,)):
                    assert tuple(t.shape) == ((M, nb * stride) if planar else (M, nb * stride, 2)) and t.dtype == dtype
                    assert not t.any()
    # an explicit stride is used as given, padded or not; one shorter than a block is refused
    for given in (5, 7, 16):
        out, d = g.streams.alloc_stream(2, 5, 3, "cpu", dtype, planar, block_stride=given)
        assert d.block_stride == given and d.ant_stride == 3 * given and d.num_samples == 5
        assert tuple((out[0] if planar else out).shape)[:2] == (2, 3 * given)
    with pytest.raises(ValueError):
        g.streams.alloc_stream(2, 5, 3, "cpu", dtype, planar, block_stride=4)


def test_alloc_stream_refuses_what_no_layout_holds(g):
    for dtype in (torch.int8, torch.int16, torch.float64):
        with pytest.raises(ValueError, match="a planar output is float32"):
            g.streams.alloc_stream(2, 5, 1, "cpu", dtype, planar=True)
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(ValueError, match="out_dtype must be torch.int8, torch.int16 or torch.float32"):
            g.streams.alloc_stream(2, 5, 1, "cpu", dtype)


@pytest.mark.parametrize("planar", (True, False))
def test_input_desc_checks_the_window_once_and_at_its_edge(g, planar):
    M, ntot = 2, 40
    signal = tuple(torch.zeros((M, ntot)) for _ in range(2)) if planar else torch.zeros((M, ntot, 2))
    for N, nb, start, stride in ((40, 1, 0, None), (10, 4, 0, None), (7, 3, 5, 14), (7, 3, 33, 0), (1, 40, 0, 1), (3, 2, 1, 36)):
        s = N if stride is None else stride
        assert start + (nb - 1) * s + N == ntot
        # the window that ends exactly at Ntot passes the check: the next refusal is signal_desc's, of a tensor off the device
        with pytest.raises(ValueError, match="must live on the HIP device"):
            g.streams.input_desc(signal, N, nb, start, stride)
        with pytest.raises(ValueError, match="shorter than"):  # one sample more, three ways
            g.streams.input_desc(signal, N + 1, nb, start, s)
        with pytest.raises(ValueError, match="shorter than"):
            g.streams.input_desc(signal, N, nb, start + 1, stride)
        if nb > 1:
            with pytest.raises(ValueError, match="shorter than"):
                g.streams.input_desc(signal, N, nb, start - (nb - 2), s + 1)
    with pytest.raises(ValueError, match="shorter than"):
        g.streams.input_desc(signal, 5, 2, 10, -1)  # a negative stride, though both blocks lie inside
    for N, nb in ((0, 1), (5, 0), (-1, 1)):
        with pytest.raises(ValueError, match="must be positive"):
            g.streams.input_desc(signal, N, nb)


def test_overlap_save_blocks_against_its_two_formulas(g):
    for total in range(1, 61):
        for T in range(1, 9):
            for B in range(1, 6):
                for D in range(1, 5):
                    Q = ((total - T) // D + 1) // B if total >= T else 0  # the filter's: Q = ((total - T) / D + 1) / B
                    for fn, args in ((g.streams.overlap_save_blocks, (total, T, D, B)), (g.filtering.stream_blocks, (total, T, D, B))):
                        if Q < 1:
                            with pytest.raises(ValueError):
                                fn(*args)
                        else:
                            assert fn(*args) == (Q * D + T - 1, Q * D, Q, B, B * Q), (total, T, D, B)
                Qout = (total - T + 1) // B if total >= T else 0  # the space-time filter's: Qout = (total - T + 1) / B
                if Qout < 1:
                    with pytest.raises(ValueError):
                        g.spacetime.stream_blocks(total, T, B)
                else:
                    assert g.spacetime.stream_blocks(total, T, B) == (Qout + T - 1, Qout, Qout, B, B * Qout), (total, T, B)
    for bad in ((10, 3, 1, 0), (10, 3, 1, -1)):
        with pytest.raises(ValueError):
            g.filtering.stream_blocks(*bad)
    for bad in ((10, 3, 0), (10, 0, 1)):
        with pytest.raises(ValueError):
            g.spacetime.stream_blocks(*bad)


@pytest.mark.parametrize("planar", (True, False))
def test_the_host_twin_accepts_an_allocated_descriptor(g, planar):
    """one tap of value 1: the filter copies its input, block by block, into the padded output"""
    M, N, B = 2, 5, 3
    rng = np.random.default_rng(5)
    x_re, x_im = (np.ascontiguousarray(rng.standard_normal((M, B * N)), dtype=np.float32) for _ in range(2))
    idesc = g.streams.host_desc(x_re, x_im, PLANAR, M, N, B * N, N)
    out, odesc = g.streams.alloc_stream(M, N, B, "cpu", planar=planar)  # Q = N - T + 1 = N
    stride = int(odesc.block_stride)
    assert stride == (8 if planar else 6)
    assert g.filter_samples_host(idesc, B, np.ones(1), odesc) == g._lib.GAT_OK
    y_re, y_im = (out[0].numpy(), out[1].numpy()) if planar else (out.numpy()[..., 0], out.numpy()[..., 1])
    for b in range(B):
        assert np.array_equal(y_re[:, b * stride:b * stride + N], x_re[:, b * N:(b + 1) * N])
        assert np.array_equal(y_im[:, b * stride:b * stride + N], x_im[:, b * N:(b + 1) * N])
        assert not y_re[:, b * stride + N:(b + 1) * stride].any() and not y_im[:, b * stride + N:(b + 1) * stride].any()
