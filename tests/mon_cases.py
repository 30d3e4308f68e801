"""What the tracking monitor's host and GPU tests share: the grid of the issue, accumulators with NaN padding between the blocks,
one flat float64 buffer holding every output between canaries (so that a call's whole effect is one array: compared at once, as
integer views), and the raw call of gat_track_monitor_host / gat_track_monitor on it."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from tests import mon_ref as ref

OVERLAYS = {"pd1": np.ones(1, np.int8), "pd2": np.array([1, -1], np.int8), "nh10": ref.NH10, "ones20": np.ones(20, np.int8), "nh20": ref.NH20}
GUARD = 4                    # canary doubles around every output
CANARY = -6.02214076e23      # one bit pattern, never a result
OUTPUTS = ("prompt_re", "prompt_im", "windows", "energy", "channels", "sym_re", "sym_im", "sym_wbp")
FORCED = 3                   # the forced stream offset of the grid (mod Pd)


def block_counts(Pd):
    return sorted({b for b in (1, Pd - 1, Pd, 2 * Pd - 2, 2 * Pd - 1, 2 * Pd, 97) if b >= 1})


def data_configs(Pd):
    """(B, K, M, weighted, L, prompt_index, stride pad) of the grid"""
    for B, K, M, wt, (L, l), pad in itertools.product(block_counts(Pd), (1, 3), (1, 3), (False, True), ((3, 1), (1, 0)), (0, 5)):
        yield B, K, M, wt, L, l, pad


def call_configs(B, Pd):
    """(W, first_block, forced or None)"""
    for W, fb, forced in itertools.product(sorted({1, 7, B, B + 3}), (0, 13), (None, FORCED % Pd)):
        yield W, fb, forced


def make_acc(rng, B, K, L, M, pad):
    """float32 accumulators: flat buffers of exactly the call's extent with NaN between the blocks, and the dense [B, K, L, M]"""
    n, stride = K * L * M, K * L * M + pad
    dense = [rng.standard_normal((B, K, L, M)).astype(np.float32) * 40.0 for _ in range(2)]
    flat = [np.full((B - 1) * stride + n, np.nan, np.float32) for _ in range(2)]
    for f, d in zip(flat, dense):
        for b in range(B):
            f[b * stride:b * stride + n] = d[b].reshape(-1)
    return flat[0], flat[1], dense[0], dense[1], stride


def make_weights(rng, K, M):
    return (rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))) / np.sqrt(M)


def layout(B, K, Pd, W, want=OUTPUTS):
    """name -> (first double, doubles) of every wanted output in the flat buffer, and the buffer's length"""
    NW, cap = (B + W - 1) // W, B // Pd
    sizes = dict(prompt_re=K * B, prompt_im=K * B, windows=K * NW * 6, energy=K * Pd, channels=K * 4, sym_re=K * cap, sym_im=K * cap, sym_wbp=K * cap)
    at, off = {}, GUARD
    for name in OUTPUTS:
        if name in want:
            at[name] = (off, sizes[name])
            off += sizes[name] + GUARD
    return at, off


def config(g, L, l, W, overlay, forced, fb):
    return g.monitor.monitor_config(L, l, W, overlay, forced, fb)


def raw_call(fn, handle, acc_re_ptr, acc_im_ptr, stride, B, K, M, cfg, w_re_ptr, w_im_ptr, out_ptr, at):
    """fn: gat_track_monitor_host (handle None) or gat_track_monitor; out_ptr: address of the flat buffer"""
    outs = [(out_ptr + 8 * at[n][0]) if n in at else None for n in OUTPUTS]
    head = (handle,) if handle is not None else ()
    return int(fn(*head, acc_re_ptr, acc_im_ptr, stride, B, K, M, C.byref(cfg) if cfg is not None else None, w_re_ptr, w_im_ptr, *outs))


def host_call(g, acc_re, acc_im, stride, B, K, M, cfg, w=None, want=OUTPUTS):
    """the twin on numpy buffers: (status, flat buffer, layout)"""
    at, total = layout(B, K, int(cfg.symbol_blocks), int(cfg.window_blocks), want)
    buf = np.full(total, CANARY)
    w_re = np.ascontiguousarray(w.real) if w is not None else None
    w_im = np.ascontiguousarray(w.imag) if w is not None else None
    rc = raw_call(g.load_library().gat_track_monitor_host, None, acc_re.ctypes.data, acc_im.ctypes.data, stride, B, K, M, cfg,
                  w_re.ctypes.data if w is not None else None, w_im.ctypes.data if w is not None else None, buf.ctypes.data, at)
    return rc, buf, at


def canaries_intact(buf, at):
    mask = np.ones(buf.size, bool)
    for off, n in at.values():
        mask[off:off + n] = False
    return bool(np.all(buf[mask] == CANARY))


def outputs_finite(buf, at, K):
    """every double of every output is finite (the records' integers are not looked at as doubles)"""
    for name in at:
        a = take(buf, at, name, K)
        fields = [a[n] for n in a.dtype.names if a.dtype[n].kind == "f"] if a.dtype.names else [a]
        if not all(np.isfinite(f).all() for f in fields):
            return False
    return True


def take(buf, at, name, K):
    from gpuacceleratedtracking_amd import _lib

    off, n = at[name]
    a = buf[off:off + n]
    if name == "windows":
        return a.view(_lib.MONITOR_WINDOW_DTYPE).reshape(K, -1)
    if name == "channels":
        return a.view(_lib.MONITOR_CHANNEL_DTYPE).reshape(K)
    return a.reshape(K, -1) if n else a.reshape(K, 0)


# ---- the receiver scene of tests/test_monitor_pipeline_gpu.py, as synthetic prompts -----------------------------------------------
# Data bits of 20 generator blocks, two patterns with 17 transitions in 21 (a bit edge is only seen where the bit changes: with the
# edge inside a block the all-ones overlay separates the right offset from its neighbour by (19.5 / 18.5)^2 on those symbols alone).
PIPELINE_BITS = (np.array([1, -1, 1, 1, -1, 1, -1, -1, 1, -1, 1, -1, -1, 1, -1, 1, 1, -1, 1, -1, 1, -1]),
                 np.array([-1, 1, -1, 1, 1, -1, 1, -1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1, -1, 1, 1]))
PIPELINE_CN0, PIPELINE_SKIP, PIPELINE_BLOCKS = 43.0, 40, 360


def edge_series(bits, first, B, frac, cn0, T, rng, phase=0.1):
    """Unit-amplitude prompts [1, B] of receiver blocks first .. first + B whose block r holds the last 1 - frac of generator block
    r and the first frac of generator block r + 1 (a receiver that starts frac of a block into the generator's stream), at C/N0
    `cn0`: where the bit changes inside a block, the block's prompt is the difference of the two shares."""
    gen = np.repeat(bits, 20).astype(np.float64)
    amp = (1.0 - frac) * gen[first:first + B] + frac * gen[first + 1:first + B + 1]
    sigma = np.sqrt(1.0 / (2.0 * T * 10.0 ** (cn0 / 10.0)))
    return (amp * np.exp(1j * phase) + sigma * (rng.standard_normal(B) + 1j * rng.standard_normal(B)))[None, :]


# The distance of both C/N0 figures from the set 43 dB-Hz on such series, measured on the FP64 restatement (tests/mon_ref.py) with
# numpy.random.default_rng(seed), seeds 0 .. 19, first = 40, B = 360, the search's own offset and one window of all blocks:
# (satellite, frac) -> (mean of nwpr - 43, largest distance of a seed from that mean, the same two for the moments estimator), dB.
# The bit edge inside a block costs about 1 dB at this transition density (0.4 dB with random bits at 40 dB-Hz, nothing with
# block-aligned bits: +0.1 dB).  tests/test_monitor_host.py recomputes them.
PIPELINE_EXPECTED = {(0, 0.25): (-0.935, 0.670, -0.984, 0.460), (0, 0.75): (-0.889, 0.392, -0.969, 0.456),
                     (1, 0.25): (-1.040, 0.458, -1.097, 0.657), (1, 0.75): (-0.879, 0.537, -1.005, 0.690)}
