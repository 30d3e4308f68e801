"""What the Python layer knows about a ``gat_signal_desc`` (include/gat.h) and the memory behind it, stated once: how a
``signal`` argument becomes a descriptor, the one window check, how a stream output is allocated, the overlap-save geometry,
the pointer arguments of the C calls and the lifetime of what a kernel reads after its call has returned.  Every operator
module builds on this one; it depends on ``_lib`` alone.

A ``signal`` argument, wherever an operator takes one: a planar pair ``(re, im)`` of float32 ``[M, Ntot]`` or one interleaved
tensor ``[M, Ntot, 2]`` of float32 / int16 / int8, on the device; block b of ``num_blocks`` starts ``start + b * block_stride``
samples in (default stride: ``num_samples``)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

_DTYPE_LAYOUT = {torch.float32: _lib.GAT_LAYOUT_INTERLEAVED, torch.int16: _lib.GAT_LAYOUT_INTERLEAVED_I16,
                 torch.int8: _lib.GAT_LAYOUT_INTERLEAVED_I8}


# ---- pointer arguments (None: a null pointer) ----------------------------------------------------------------------------------
def vp(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def addr(a):
    """The address of a numpy array's first element."""
    return None if a is None else a.ctypes.data


def ref(s):
    return None if s is None else C.byref(s)


def planes(z: torch.Tensor, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    if z.is_complex():
        return z.real.to(dtype).contiguous(), z.imag.to(dtype).contiguous()
    return z.to(dtype).contiguous(), torch.zeros_like(z, dtype=dtype).contiguous()


def keep_alive(result, *tensors):
    """Pin the temporaries a call made (weights, taps, records, contiguous copies) to what it returns -- the descriptor where one
    is returned, otherwise the first tensor (``result``: that object, or the tuple it is first in): the kernel reads them after the
    call has returned.  On a context bound to torch's current stream the caching allocator's stream ordering would cover a
    temporary freed at once; on ``Context(stream="own")``, or on any stream other than the current one, nothing does, and the
    memory could be handed out again before the kernel ran."""
    (result[0] if isinstance(result, tuple) else result)._keep = tensors
    return result


# ---- descriptors ---------------------------------------------------------------------------------------------------------------
def signal_desc(re: torch.Tensor, im: torch.Tensor | None, num_samples: int, start: int = 0,
                block_stride: int | None = None, per_channel: bool = False) -> _lib.SignalDesc:
    """Describe a planar float32 pair [(K,) M, Ntot] or an interleaved tensor [(K,) M, Ntot, 2] of
    float32 (ComplexF32), int16 or int8 {re, im} pairs."""
    il = im is None
    t = re
    if not t.is_cuda:
        raise ValueError("signal must live on the HIP device")
    if il:
        if t.dtype not in _DTYPE_LAYOUT:
            raise ValueError("interleaved signal must be float32, int16 or int8")
        if t.shape[-1] != 2 or t.stride(-1) != 1 or t.stride(-2) != 2:
            raise ValueError("interleaved signal must be [..., N, 2] with unit inner strides")
        dims = t.dim() - 1
        stride = lambda d: t.stride(d - 1) // 2  # noqa: E731  (in complex samples)
        ntot = t.shape[-2]
        layout = _DTYPE_LAYOUT[t.dtype]
    else:
        if t.dtype != torch.float32 or im.dtype != torch.float32:
            raise ValueError("planar signal planes must be float32")
        if t.stride(-1) != 1 or im.stride() != t.stride() or im.shape != t.shape:
            raise ValueError("planar signal planes must be sample-contiguous with equal strides")
        dims = t.dim()
        stride = lambda d: t.stride(d)  # noqa: E731
        ntot = t.shape[-1]
        layout = _lib.GAT_LAYOUT_PLANAR
    if start < 0 or start + num_samples > ntot:
        raise ValueError("signal_start_sample/num_samples outside the signal")
    d = _lib.SignalDesc()
    off = start * (_lib.SAMPLE_BYTES[layout] if il else 4)
    d.re = t.data_ptr() + off
    d.im = None if il else im.data_ptr() + off
    d.layout = layout
    d.num_samples = num_samples
    d.num_ants = t.shape[dims - 2] if dims >= 2 else 1
    d.ant_stride = stride(-2) if dims >= 2 else ntot
    d.block_stride = num_samples if block_stride is None else block_stride
    d.chan_stride = stride(-3) if (per_channel and dims >= 3) else 0
    return d


def input_desc(signal, num_samples: int, num_blocks: int, start: int = 0, block_stride: int | None = None):
    """``(first tensor, descriptor)`` of a ``signal`` argument (the module's docstring says what one is), after the one check
    that its ``num_blocks`` blocks lie inside the tensor."""
    re, im = signal if isinstance(signal, (tuple, list)) else (signal, None)
    nb, N = int(num_blocks), int(num_samples)
    if nb < 1 or N < 1:
        raise ValueError("num_blocks and num_samples must be positive")
    stride = N if block_stride is None else int(block_stride)
    ntot = re.shape[-2] if im is None else re.shape[-1]
    if stride < 0 or start + (nb - 1) * stride + N > ntot:
        raise ValueError("signal shorter than start + (num_blocks - 1) * block_stride + num_samples")
    return re, signal_desc(re, im, N, start=int(start), block_stride=stride)


def output_desc(out, num_samples: int, block_stride: int | None = None) -> _lib.SignalDesc:
    """A caller's own output -- a planar pair or one interleaved tensor -- described as it is (default stride: ``num_samples``)."""
    o_re, o_im = out if isinstance(out, (tuple, list)) else (out, None)
    return signal_desc(o_re, o_im, num_samples, block_stride=num_samples if block_stride is None else int(block_stride))


def _plane_bytes(layout: int) -> int:
    """Bytes from one sample to the next in a plane of this layout (an unknown layout is the callee's to refuse)."""
    return 4 if layout == _lib.GAT_LAYOUT_PLANAR else _lib.SAMPLE_BYTES.get(layout, 1)


def host_desc(arr, im, layout: int, M: int, N: int, ant_stride: int, block_stride: int, offset: int = 0) -> _lib.SignalDesc:
    """A descriptor of HOST memory over numpy arrays, for the library's host twins; ``offset`` samples into them."""
    step = _plane_bytes(layout)
    return _lib.SignalDesc(arr.ctypes.data + offset * step, None if im is None else im.ctypes.data + offset * step, layout, M, N,
                           ant_stride, block_stride, 0)


def alloc_stream(num_ants: int, num_samples: int, num_blocks: int, device, dtype=torch.float32, planar: bool = False,
                 block_stride: int | None = None, zero: bool = True):
    """A stream output and its descriptor, ``(tensor, desc)``: one interleaved tensor ``[M, Ntot, 2]`` of ``dtype`` or, with
    ``planar=True``, a float32 ``(re, im)`` pair ``[M, Ntot]``, ``Ntot = num_blocks * block_stride``.  ``block_stride=None``:
    ``num_samples`` rounded up to 16 bytes, so that every block starts on a 16-byte boundary -- what lets the plan
    (``blocks_aligned``, csrc/gat_sig_plan.h) pick the tiled and streaming kernels; what lies between blocks is zero
    (``zero=False``: uninitialised, like everything else).  An explicit ``block_stride`` is used as given."""
    if planar:
        if dtype != torch.float32:
            raise ValueError("a planar output is float32")
        layout = _lib.GAT_LAYOUT_PLANAR
    elif dtype in _DTYPE_LAYOUT:
        layout = _DTYPE_LAYOUT[dtype]
    else:
        raise ValueError("out_dtype must be torch.int8, torch.int16 or torch.float32")
    M, N, nb = int(num_ants), int(num_samples), int(num_blocks)
    if block_stride is None:
        vs = 16 // _plane_bytes(layout)  # samples per 16 bytes: 4 planar float32, 2 ComplexF32, 4 int16 pairs, 8 int8 pairs
        stride = (N + vs - 1) // vs * vs
    else:
        stride = int(block_stride)
        if stride < N:
            raise ValueError("block_stride shorter than num_samples")
    ld = nb * stride
    alloc = torch.zeros if zero else torch.empty
    if planar:
        out = (alloc((M, ld), dtype=dtype, device=device), alloc((M, ld), dtype=dtype, device=device))
        return out, _lib.SignalDesc(out[0].data_ptr(), out[1].data_ptr(), layout, M, N, ld, stride, 0)
    out = alloc((M, ld, 2), dtype=dtype, device=device)
    return out, _lib.SignalDesc(out.data_ptr(), None, layout, M, N, ld, stride, 0)


def stream_views(out, num_samples: int):
    """The first ``num_samples`` samples of every row of an allocation of ``alloc_stream``: what the ``*_stream`` operators return of
    their one block (the rows stay padded to 16 bytes, so that an aligned input runs the tiled kernel)."""
    return tuple(p[:, :num_samples] for p in out) if isinstance(out, tuple) else out[:, :num_samples]


def overlap_save_blocks(total_samples: int, num_taps: int, decimation: int, num_blocks: int):
    """Overlap-save geometry of a contiguous stream of ``total_samples`` behind ``num_taps`` taps and a decimation:
    ``(N, in_stride, Q, B, outputs)`` -- B blocks of N = Q D + T - 1 input samples every Q D samples give Q outputs each,
    ``outputs = B Q`` in all (the stream's own (total - T) / D + 1, rounded down to a multiple of B)."""
    T, D, B = int(num_taps), int(decimation), int(num_blocks)
    Q = ((int(total_samples) - T) // D + 1) // B
    if Q < 1:
        raise ValueError("more blocks than outputs")
    return Q * D + T - 1, Q * D, Q, B, B * Q
