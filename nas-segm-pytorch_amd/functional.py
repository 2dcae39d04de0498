"""Differentiable host-side wrappers of the nasseg HIP kernels.

Each function here is one ``torch.autograd.Function`` whose forward and backward
are calls into libnasseg_hip.so (see include/nasseg.h).  PyTorch supplies device
memory (caching allocator), the current HIP stream and the autograd tape only;
no ATen compute op runs on the hot path.  Tensors keep the reference's NCHW
*shape* but live in ``torch.channels_last`` memory, which is the NHWC layout the
kernels address directly.
"""
import collections
import ctypes
import os
import weakref

import numpy as np
import torch

from ._lib import LaunchProfiler, NassegError, current_stream, lib, ptr, require_device

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
RED_SUM, RED_SUMSQ, RED_DOT2, RED_DOT1 = 0, 1, 3, 4


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
_BF16_PREFIX = "nasseg_bf16_"


def _k(name, t):
    """Entry point for activations stored like ``t``: nasseg_<op> (fp32) or its bfloat16 twin
    nasseg_bf16_<op> (same arguments; include/nasseg.h)."""
    if t.dtype == torch.float32:
        return name
    return _BF16_PREFIX + name[7:]


def _to_dtype(t, dtype):
    """t.to(dtype) between fp32 and bf16 as a nasseg launch (nasseg_to_bf16 / nasseg_from_bf16: the same rounding as
    torch's; an ATen kernel inside a recorded step would be a barrier for engine/graph_dag.py); anything else:
    torch's .to()"""
    if t.dtype == dtype:
        return t
    t = t.contiguous()
    if t.is_cuda and t.numel() and (t.dtype, dtype) in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
        y = torch.empty_like(t, dtype=dtype)
        lib.call("nasseg_to_bf16" if dtype == torch.bfloat16 else "nasseg_from_bf16", ptr(t), ptr(y), t.numel(),
                 current_stream())
        return y
    return t.to(dtype)


def _cl(x):
    """NHWC-contiguous view/copy of a 4-D NCHW-shaped activation (fp32 or bf16 storage)."""
    require_device(x)
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NassegError("nasseg activations are fp32 or bf16 (got {})".format(x.dtype))
    if x.dim() != 4:
        raise NassegError("expected a 4-D activation, got shape {}".format(tuple(x.shape)))
    return x.contiguous(memory_format=torch.channels_last)


def _new(like, B, C, H, W):
    return torch.empty((B, C, H, W), device=like.device, dtype=like.dtype,
                       memory_format=torch.channels_last)


def _ws(like, n):
    return torch.empty((max(int(n), 1),), device=like.device, dtype=torch.float32)


def _vec(like, n):
    return torch.empty((int(n),), device=like.device, dtype=torch.float32)


def _rows_ws(like, n, C):
    """Partial rows of a per-channel pair of sums: n rows of 2 C floats, plus 64 rows that nasseg_rows_sum /
    nasseg_bn_finalize use as the scratch of their two-level reduction (include/nasseg.h, csrc/reduce.hip)"""
    return _ws(like, (n + 64) * 2 * C)


def _bn_parts(stats, n):
    """(mean, invstd, scale, shift): the views of a statistics vector mean | invstd | scale | shift of n channels"""
    return stats[0:n], stats[n:2 * n], stats[2 * n:3 * n], stats[3 * n:]


def _scale_shift(stats, n):
    """(scale, shift) of a statistics vector - (None, None) without one: nothing to apply on load"""
    return (None, None) if stats is None else (stats[2 * n:3 * n], stats[3 * n:])


def _bn_alloc(like, C, training, M, shape):
    """First half of the forward BatchNorm head: torch's check (same condition, exception class and text as
    torch.nn.functional.batch_norm), then (stats, its views (mean, invstd, scale, shift)), still to be filled"""
    if training and M <= 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(
            tuple(shape)))
    stats = _vec(like, 4 * C)
    return stats, _bn_parts(stats, C)


def _bn_fill(parts, C, M, bn, training, momentum, eps, x=None, rows=None):
    """Second half: fill ``parts`` = (mean, invstd, scale, shift) - views of C channels, of a wider vector too - from
    what the caller has.  Training: the statistics of the M x C tensor ``x`` by a reduction over it, or of the partial
    rows an epilogue left, ``rows`` = (buffer, count); both move the running buffers of bn = (gamma, beta,
    running_mean, running_var, num_batches_tracked).  Otherwise the running statistics."""
    gamma, beta, rm, rv, nbt = bn
    mean, invstd, scale, shift = parts
    s = current_stream()
    if not training:
        lib.call("nasseg_bn_eval_params", C, float(eps), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(mean),
                 ptr(invstd), ptr(scale), ptr(shift), s)
    elif rows is not None:
        lib.call("nasseg_bn_finalize", ptr(rows[0]), rows[1], M, C, float(eps), float(momentum), ptr(gamma),
                 ptr(beta), ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(rm), ptr(rv), ptr(nbt), s)
    else:
        ws = _ws(x, lib.query("nasseg_colred_workspace", 1, M, C))
        lib.call(_k("nasseg_bn_stats", x), ptr(x), C, M, C, float(eps), float(momentum), ptr(gamma), ptr(beta),
                 ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(rm), ptr(rv), ptr(nbt), ptr(ws), s)


def _bn_head(like, C, M, shape, bn, training, momentum, eps, x=None, rows=None):
    """The forward BatchNorm head in one step: (stats, mean, invstd, scale, shift) of C channels over M pixels"""
    stats, parts = _bn_alloc(like, C, training, M, shape)
    _bn_fill(parts, C, M, bn, training, momentum, eps, x, rows)
    return (stats,) + parts


# BatchNorm backward whose apply kernel adds up the partial rows of its sums itself (nasseg_bn_bwd_apply_rows): on the
# small maps of the CVPR cells the sums come as 8 - 128 rows (the first stage of the reduction over gradient and conv
# output, or the statistics rows of a fused backward-data kernel), and the launch that summed them - colred_finalize /
# rows_group_sum, ~5 us on the dependency chain of every BatchNorm backward, 81 + 60 of the ~1000 kernels of a replayed
# CVPR 321x321 step - is replaced by one more round trip to L2 at the head of the apply kernel.  Rows beyond
# nasseg_bn_bwd_apply_rows_max_bytes() keep the summing launch.  NASSEG_APPLY_ROWS=0 restores it everywhere (A/B).
APPLY_ROWS = os.environ.get("NASSEG_APPLY_ROWS", "1") != "0"


def _rows_small(nrows, C):
    """few enough rows of 2 C floats for every workgroup of the apply kernel to add them up itself"""
    return (APPLY_ROWS and C % 4 == 0 and C <= 1024 and 0 < nrows
            and nrows * 2 * C * 4 <= lib.query("nasseg_bn_bwd_apply_rows_max_bytes"))


def _bn_bwd_apply(g, z, scale, shift, mean, invstd, sums, M, C, training, act, dz, rows=None):
    """dz of a BatchNorm (+ activation) backward from the summed sums, or - rows = (buffer, count) - from their
    partial rows (``sums`` then RECEIVES the totals: they are the BatchNorm's parameter gradients)"""
    if rows is not None:
        lib.call(_k("nasseg_bn_bwd_apply_rows", g), ptr(g), ptr(z), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                 ptr(rows[0]), rows[1], ptr(sums), M, C, int(training), act, ptr(dz), current_stream())
    else:
        lib.call(_k("nasseg_bn_bwd_apply", g), ptr(g), ptr(z), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                 ptr(sums), M, C, int(training), act, ptr(dz), current_stream())
    return dz


def _bn_bwd_reduce(g, z, scale, shift, mean, invstd, act, sums, M, C, for_apply):
    """{sum g', sum g' * xhat} of a BatchNorm backward over the M pixels of g, z: into ``sums`` (returns None), or -
    when the caller goes on to _bn_bwd_apply (for_apply) and the first stage leaves few rows - only the rows, which
    are returned as (buffer, count) for the apply kernel to add up"""
    ws = _ws(z, lib.query("nasseg_colred_workspace", 1, M, C))
    if for_apply:
        nrows = lib.query("nasseg_colred_rows", 1, M, C)
        if _rows_small(nrows, C):
            lib.call(_k("nasseg_bn_bwd_reduce_rows", g), ptr(g), C, ptr(z), C, M, C, ptr(scale), ptr(shift), ptr(mean),
                     ptr(invstd), act, ptr(ws), current_stream())
            return ws, nrows
    lib.call(_k("nasseg_bn_bwd_reduce", g), ptr(g), C, ptr(z), C, M, C, ptr(scale), ptr(shift), ptr(mean),
             ptr(invstd), act, ptr(sums), ptr(ws), current_stream())
    return None


# ---------------------------------------------------------------------------
# deferred finalisation of weight gradients
# ---------------------------------------------------------------------------
class deferred_wgrad(object):
    """``with F.deferred_wgrad(): loss.backward()``

    A weight gradient is a two-stage reduction (per-slab partial sums, then their sum) and only
    the optimiser reads it.  Inside this context the backward-weight calls stop after stage one
    and the second stages of ALL layers run when the context exits - one launch per 16 layers
    (nasseg_wgrad_finalize_many) instead of one small launch per layer on the backward chain.
    Opt-in, because between backward and the exit the gradient tensors are allocated but not yet
    written: the caller must have cleared the gradients and every weight must be used once in
    the graph (autograd then just adopts the new tensor; an accumulation - or the copy it makes
    of a tensor somebody else still references, which is why only the ADDRESS is queued here -
    would read it too early), and must not touch ``param.grad`` before the exit.
    Same arithmetic in the same order: results are bit-identical."""

    active = False
    pending = []   # (partials, address of the gradient tensor, finalisation dims)
    grouped = {}   # (entry point, dtype) -> [(tensors the kernels read, launch arguments)]: first
    #                stages of small layers, launched side by side at the exit
    #                (nasseg_conv_wgrad_many / nasseg_dwconv_wgrad_many)
    side_ok = False  # first stages may go to a second stream (WGRAD_STREAM; never while a hipGraph is captured)
    side_used = {}   # device -> that stream, once a launch went there

    def __init__(self, enabled=True, params=None, second_stream=True):
        """params: the parameters being trained; when given, the exit verifies that every
        deferred gradient is the tensor autograd adopted as some ``param.grad`` (it would be a
        copy - of unwritten memory - had a condition above been violated) and fails loudly.
        second_stream: first stages may be launched on a second stream (WGRAD_STREAM below)."""
        self.enabled = bool(enabled)
        self.params = params
        self.second_stream = bool(second_stream)

    def __enter__(self):
        self.prev = deferred_wgrad.active, deferred_wgrad.side_ok
        deferred_wgrad.active = self.enabled
        deferred_wgrad.side_ok = bool(self.enabled and self.second_stream and WGRAD_STREAM and torch.cuda.is_available()
                                      and not torch.cuda.is_current_stream_capturing())
        return self

    @staticmethod
    def _launch_group(entry, dtype, calls, stream):
        flat = [v for c in calls for v in c[1]]
        table = (ctypes.c_int64 * len(flat))(*flat)
        name = entry if dtype == torch.float32 else entry.replace("nasseg_", "nasseg_bf16_", 1)
        if lib.recorder is not None:  # (a step being recorded: c[0] = (input, dz, prologue scale, shift, partials))
            lib.recorder.annotate(reads=[t for c in calls for t in c[0][:4]], writes=[c[0][4] for c in calls])
        lib.call(name, len(calls), table, stream)

    @staticmethod
    def _finalize(todo, stream):
        """second stages of the layers in ``todo`` (partials, address of the gradient, dims) on ``stream``"""
        n = len(todo)
        parts = (ctypes.c_void_p * n)(*[ptr(ws) for ws, _, _ in todo])
        outs = (ctypes.c_void_p * n)(*[addr for _, addr, _ in todo])
        dims = (ctypes.c_int * (5 * n))()
        for j, (_, _, d) in enumerate(todo):
            dims[5 * j:5 * j + 5] = d
        if lib.recorder is not None:  # (dims: rows, taps, N, K, flat - the gradient tensor has taps * N * K floats)
            lib.recorder.annotate(reads=[ws for ws, _, _ in todo],
                                  writes=[(addr, 4 * d[1] * d[2] * d[3]) for _, addr, d in todo])
        lib.call("nasseg_wgrad_finalize_many", n, parts, outs, dims, stream)

    def __exit__(self, exc_type, exc, tb):
        deferred_wgrad.active, deferred_wgrad.side_ok = self.prev
        todo, deferred_wgrad.pending = deferred_wgrad.pending, []
        groups, deferred_wgrad.grouped = deferred_wgrad.grouped, {}
        sides, deferred_wgrad.side_used = deferred_wgrad.side_used, {}
        if exc_type is None:
            for (entry, dtype), calls in groups.items():
                self._launch_group(entry, dtype, calls, current_stream())
                todo.extend(c[2] for c in calls)
        # the second stream's launches fill the partial sums finalised below: join (also after an exception)
        for dev, side in sides.items():
            torch.cuda.current_stream(dev).wait_stream(side)
        if exc_type is None:
            if todo:
                self._finalize(todo, current_stream())
            if self.params is not None and todo:
                adopted = set(p.grad.data_ptr() for p in self.params if p.grad is not None)
                if any(addr not in adopted for _, addr, _ in todo):
                    raise NassegError("deferred_wgrad: autograd copied a weight gradient before it was "
                                      "finalised (gradients not cleared, or a weight used twice?)")
        return False


# largest x + dy footprint (bytes) of a layer whose backward-weight launch is grouped
_GROUP_WGRAD_BYTES = 48 << 20

# Weight gradients on a second stream.  Inside deferred_wgrad nothing on the backward chain waits for a weight
# gradient: its first stage reads the layer's input and the gradient w.r.t. its output, writes partial sums, and the
# second stage runs at the exit.  Launched on the stream of the chain, those kernels sit between the backward-data
# kernels - or, the grouped small layers, behind the whole backward - although many of them have too few workgroups
# to fill 256 CUs; on a stream of their own (which first waits for what the chain has launched so far) the GPU runs
# them beside the chain, and the chain's stream waits for that stream once, at the exit.  Bits of NASSEG_WGRAD_STREAM:
# 1 = the launches of large layers, 2 = the grouped small layers, _SIDE_GROUP at a time as they come.  Measured on one
# box (profiles/r05_ab_second_half_same_box.txt): either bit alone is level, both together +0.5 % on the headline
# step and +1.2 - 1.5 % on WACV arch1.  0: everything on the chain's stream (A/B).  Never while a hipGraph is being
# captured (one second stream inside a capture made the replay slower, two crash this runtime: DESIGN_HISTORY.md),
# and only where the caller asks for it (deferred_wgrad(second_stream=...): a step that is launch-bound on the host
# gains nothing from more launches - CVPR 321x321 from the host 750.5 / 745.8).  The second stages stay on the chain's
# stream, after the join: sixteen at a time on the second stream as backward goes measured level (281.1 / 281.4).
# Same kernels on the same data: bit-identical.
WGRAD_STREAM = int(os.environ.get("NASSEG_WGRAD_STREAM", "3"))
_SIDE_STREAMS = {}
_SIDE_GROUP = int(os.environ.get("NASSEG_WGRAD_SIDE_GROUP", "8"))
# (in a step being recorded for lanes: measured slower at 8 and level at 16 - more launches of the grouped kernels -,
#  profiles/r06_ab_lanes.txt; kept as a switch)
_RECORD_GROUP = int(os.environ.get("NASSEG_WGRAD_RECORD_GROUP", "1000000"))


def _wgrad_stream(t, keep):
    """the stream a first-stage weight-gradient launch over ``t`` goes to, after it has been made to wait for the
    current one: the second stream (``keep`` - the tensors the launch touches, or the queued calls of a grouped launch -
    is then recorded on it for the allocator), else the current"""
    if not (deferred_wgrad.side_ok and t.is_cuda and (WGRAD_STREAM & 1 or isinstance(keep, list))):
        return current_stream()
    side = deferred_wgrad.side_used.get(t.device)
    if side is None:
        side = _SIDE_STREAMS.get(t.device)
        if side is None:
            side = _SIDE_STREAMS[t.device] = torch.cuda.Stream(t.device)
            LaunchProfiler.streams[side.cuda_stream] = side
        deferred_wgrad.side_used[t.device] = side
    side.wait_stream(torch.cuda.current_stream(t.device))
    # What the launch reads and writes must not be handed out again before the second stream is through with it -
    # and must not stay allocated until the end of backward either (round 5 kept references until the exit: peak
    # memory of a large step grew towards activations + every dz).  record_stream tells the caching allocator
    # exactly that: the block is reusable once the second stream has passed the point where it was freed.
    for item in (keep if isinstance(keep, tuple) else [x for c in keep for x in c[0]]):
        if item is not None:
            item.record_stream(side)
    return side.cuda_stream


def _group_wgrad(entry, cur, tensors, desc, fin):
    """queue a small layer's first stage (``fin``: what its second stage needs, queued once the first is launched);
    with WGRAD_STREAM & 2, launch the queue on the second stream when it holds _SIDE_GROUP layers (a list as ``keep``
    marks such a launch for _wgrad_stream)"""
    key = (entry, cur.dtype)
    calls = deferred_wgrad.grouped.setdefault(key, [])
    calls.append((tensors, desc, fin))
    if WGRAD_STREAM & 2 and deferred_wgrad.side_ok and cur.is_cuda and len(calls) >= _SIDE_GROUP:
        del deferred_wgrad.grouped[key]
        deferred_wgrad._launch_group(entry, cur.dtype, calls, _wgrad_stream(cur, calls))
        deferred_wgrad.pending.extend(c[2] for c in calls)
    elif lib.recorder is not None and len(calls) >= _RECORD_GROUP:
        # a step being recorded for replay in lanes (engine/graph_dag.py): _SIDE_GROUP layers at a time as backward
        # goes, on the recording stream - the layout then runs such a launch beside the NEXT piece of the backward
        # chain; one launch of all of them behind the chain would be a stage of its own
        del deferred_wgrad.grouped[key]
        deferred_wgrad._launch_group(entry, cur.dtype, calls, current_stream())
        deferred_wgrad.pending.extend(c[2] for c in calls)


def _dw_wgrad(cur, dz, w, psc, psh, pact, geom):
    """Weight gradient of a depthwise conv (geom = B, H, W, C, Ho, Wo, k, stride, pad, dil); see
    _dense_wgrad."""
    B, H, W, C, Ho, Wo, k, stride, pad, dil = geom
    dwt = torch.empty_like(w)
    ws = _ws(cur, lib.query("nasseg_dwconv_wgrad_workspace", B, C, Ho, Wo, k))
    if deferred_wgrad.active and (B * H * W * C + B * Ho * Wo * C) * cur.element_size() <= _GROUP_WGRAD_BYTES:
        desc = (ptr(cur), ptr(dz), ptr(ws), ptr(psc) or 0, ptr(psh) or 0, pact) + tuple(geom)
        _group_wgrad("nasseg_dwconv_wgrad_many", cur, (cur, dz, psc, psh, ws), desc, _fin_entry(ws, dwt, k * k, C, 1, 0))
        return dwt
    st = _wgrad_stream(cur, (cur, dz, psc, psh, ws))  # (before this layer is queued for finalisation)
    lib.call(_k("nasseg_dwconv_wgrad", cur), ptr(cur), ptr(dz), _finish_wgrad(ws, dwt, k * k, C, 1, 0), ptr(ws),
             ptr(psc), ptr(psh), pact, *geom, st)
    return dwt


def _dense_wgrad(cur, dz, w, psc, psh, pact, geom):
    """Weight gradient of a dense conv (geom = B, Hs, Ws, K, Ho, Wo, N, kh, kw, stride, pad, dil),
    ``cur`` read through the prologue (psc, psh, pact).  Immediate, or - inside deferred_wgrad -
    with its second stage deferred and, for small maps, its first stage grouped as well."""
    B, Hs, Ws, K, Ho, Wo, N, kh, kw, stride, pad, dil = geom
    dwt = torch.empty_like(w)
    ws = _ws(cur, lib.query("nasseg_conv_wgrad_workspace", B, Ho, Wo, N, K, kh, kw))
    flat = int(lib.query("nasseg_conv_fwd_pack_mode", K, kh, kw) == 2)
    # (layers that nasseg_conv_wgrad runs on its LDS-tiled 3x3 kernel are not grouped: the grouped launch always
    #  uses the generic kernel, and deferred / immediate finalisation must give the same bits)
    if (deferred_wgrad.active and (B * Hs * Ws * K + B * Ho * Wo * N) * cur.element_size() <= _GROUP_WGRAD_BYTES
            and not (psc is None and psh is None and not pact
                     and lib.query("nasseg_conv_wgrad_lds3x3", B, Hs, Ws, K, Ho, Wo, N, kh, kw, stride, pad, dil))):
        desc = (ptr(cur), K, ptr(dz), N, ptr(ws), ptr(psc) or 0, ptr(psh) or 0, pact) + tuple(geom)
        _group_wgrad("nasseg_conv_wgrad_many", cur, (cur, dz, psc, psh, ws), desc,
                     _fin_entry(ws, dwt, kh * kw, N, K, flat))
        return dwt
    st = _wgrad_stream(cur, (cur, dz, psc, psh, ws))  # (before this layer is queued for finalisation)
    lib.call(_k("nasseg_conv_wgrad", cur), ptr(cur), K, ptr(dz), N, _finish_wgrad(ws, dwt, kh * kw, N, K, flat),
             ptr(ws), ptr(psc), ptr(psh), pact, *geom, st)
    return dwt


def _pw_bwd_slabs(kind, cur, z, w, stride, pad, need_dw, need_dx, i, ops):
    """> 0: this op's whole backward (BatchNorm backward on load, weight gradient, input gradient)
    runs as ONE kernel, nasseg_conv_pw_bwd_bn (the value is its number of partial rows): a
    pointwise conv with a BatchNorm behind it, both gradients wanted, a map large enough to fill
    the GPU with slabs, and NO BatchNorm of the chain in front of it whose backward the separate
    backward-data kernel would fuse into its epilogue (an activation applied on load to the
    chain's input - pre_clf's ReLU - is handled: the kernel masks dx with its derivative)."""
    if not (FUSE_PW_BWD and kind == "dense" and need_dw and need_dx):
        return 0
    N, K, kh, kw = w.shape
    if not (kh == 1 and kw == 1 and stride == 1 and pad == 0):
        return 0
    if (cur.numel() + z.numel()) * cur.element_size() <= _PW_BWD_MIN_BYTES:
        return 0
    if K % 4 == 0 and i > 0 and ops[i - 1].has_bn and not (N >= K and K <= 64):
        # bn_prev in _ConvChain.backward: the producer's BatchNorm backward goes with the backward-data
        # kernel (statistics epilogue) - except where this conv widens (N >= K): there the one kernel plus
        # a bn_bwd_reduce pass over the K-channel gradient moves fewer bytes (4K + 2N per pixel) than
        # weight-gradient + backward-data with dz in between (3K + 4N): 16 -> 96 behind a BatchNorm,
        # which is what MobileNetV2's merged stem / stage-1 / stage-2 chain contains
        return 0
    B, _, H, W = cur.shape
    if K > 64 and not (_PW_BWD_WIDE and B * H * W >= _PW_BWD_WIDE_MIN_PIXELS):
        return 0
    return lib.query("nasseg_conv_pw_bwd_slabs", B, H, W, K, N)


FUSE_DW_BWD = os.environ.get("NASSEG_FUSE_DW_BWD", "1") != "0"
_DW_BWD_MIN_BYTES = int(os.environ.get("NASSEG_DW_BWD_MIN_BYTES", 24 << 20))
_FLAT_WGRAD_BN_MIN_BYTES = 24 << 20  # (output map of the stem above which its BatchNorm backward rides on the wgrad loads)


def _dw_bwd_rows(kind, cur, z, w, stride, pad, dil, need_dw, need_dx, i, ops):
    """> 0: this depthwise op's whole backward runs as ONE kernel, nasseg_dwconv_bwd_bn (the value
    is its number of partial rows): 3x3, between two BatchNorms of the chain (the previous op has
    one - InvertedResidual's expansion), both gradients wanted, a large map."""
    if not (FUSE_DW_BWD and kind == "dw" and need_dw and need_dx and i > 0 and ops[i - 1].has_bn):
        return 0
    if (cur.numel() + z.numel()) * cur.element_size() <= _DW_BWD_MIN_BYTES:
        return 0
    B, C, H, W = cur.shape
    return lib.query("nasseg_dwconv_bwd_bn_rows", B, C, H, W, w.shape[-1], stride, pad, dil)


def _flat_bn_ok(kind, need_dw, need_dx, psc, psh, pact, w, N, z):
    """the stem's weight gradient with the BatchNorm backward on its loads (nasseg_conv_wgrad_bn_flat)"""
    return (kind == "dense" and need_dw and not need_dx and psc is None and psh is None and not pact
            and w.shape[2] * w.shape[3] > 1 and N % 4 == 0
            and lib.query("nasseg_conv_fwd_pack_mode", w.shape[1], w.shape[2], w.shape[3]) == 2
            and z.numel() * z.element_size() > _FLAT_WGRAD_BN_MIN_BYTES)


def _wgrad_bn_ok(kind, cur, z, w, stride, pad, dil):
    """Can this layer's weight-gradient kernel apply the BatchNorm backward on load
    (nasseg_conv_wgrad_bn / nasseg_dwconv_wgrad_bn)?  Large maps only: the launches of small ones
    are grouped at the end of backward, after the backward-data kernels that need dz.  (The rule
    must not depend on whether finalisation is deferred: both ways give the same bits.)"""
    if (cur.numel() + z.numel()) * cur.element_size() <= _GROUP_WGRAD_BYTES:
        return False
    K, N = cur.shape[1], z.shape[1]
    if kind == "dw":
        return K % 4 == 0 and bool(lib.query("nasseg_dwconv_strip_ok", w.shape[-1], stride, dil))
    return (w.shape[2] == 1 and w.shape[3] == 1 and stride == 1 and pad == 0 and K % 4 == 0 and N % 4 == 0)


def _wgrad_bn(kind, cur, g, z, w, psc, psh, pact, bn, geom):
    """Weight gradient of a conv followed by BatchNorm, from the masked gradient ``g`` w.r.t. the
    BatchNorm output: returns (dw, dz); bn = (scale, shift, mean, invstd, sums, training, act) with
    act = the activation whose mask g still lacks (ACT_NONE: g arrived masked, or no activation)."""
    scale, shift, mean, invstd, sums, training, act = bn
    dz = torch.empty_like(z)
    dwt = torch.empty_like(w)
    if kind == "dw":
        B, H, W, C, Ho, Wo, k, stride, pad, dil = geom
        ws = _ws(cur, lib.query("nasseg_dwconv_wgrad_workspace", B, C, Ho, Wo, k))
        lib.call(_k("nasseg_dwconv_wgrad_bn", cur), ptr(cur), ptr(g), ptr(z), ptr(dz),
                 _finish_wgrad(ws, dwt, k * k, C, 1, 0), ptr(ws), ptr(psc), ptr(psh), pact, ptr(scale), ptr(shift),
                 ptr(mean), ptr(invstd), ptr(sums), int(training), act, *geom, current_stream())
    else:
        B, H, W, K, N = geom
        ws = _ws(cur, lib.query("nasseg_conv_wgrad_workspace", B, H, W, N, K, 1, 1))
        lib.call(_k("nasseg_conv_wgrad_bn", cur), ptr(cur), K, ptr(g), N, ptr(z), N, ptr(dz), N,
                 _finish_wgrad(ws, dwt, 1, N, K, 0), ptr(ws), ptr(psc), ptr(psh), pact, ptr(scale), ptr(shift),
                 ptr(mean), ptr(invstd), ptr(sums), int(training), act, B, H, W, K, N, current_stream())
    return dwt, dz


def _finish_wgrad(ws, dw, taps, N, K, flat):
    """Returns the pointer to pass as ``dw`` to a backward-weight entry point: the tensor itself,
    or NULL with the second stage queued when finalisation is deferred."""
    if not deferred_wgrad.active:
        return ptr(dw)
    deferred_wgrad.pending.append(_fin_entry(ws, dw, taps, N, K, flat))
    return None


def _fin_entry(ws, dw, taps, N, K, flat):
    return (ws, dw.data_ptr(), (ws.numel() // (taps * N * K), taps, N, K, flat))


def conv_out_size(size, k, stride, pad, dil):
    return (size + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _colred(mode, a, lda, b, ldb, c, ldc, S, R, C, mul=1.0):
    """[S][nacc][C] sums; nacc = 2 for SUMSQ / DOT2."""
    nacc = 2 if mode in (RED_SUMSQ, RED_DOT2) else 1
    out = _vec(a, S * nacc * C)
    ws = _ws(a, lib.query("nasseg_colred_workspace", S, R, C))
    lib.call(_k("nasseg_colred", a), mode, ptr(a), lda, ptr(b), ldb, ptr(c), ldc, ptr(out), ptr(ws),
             S, R, C, float(mul), current_stream())
    return out


def _affine_act(x, scale, shift, res, act):
    B, C, H, W = x.shape
    y = _new(x, B, C, H, W)
    lib.call(_k("nasseg_affine_act", x), ptr(x), ptr(scale), ptr(shift), ptr(res), ptr(y), x.numel(), C,
             act, current_stream())
    return y


def _axpby(a, b, alpha, beta, act=ACT_NONE):
    B, C, H, W = a.shape
    y = _new(a, B, C, H, W)
    lib.call(_k("nasseg_axpby", a), ptr(a), ptr(b), ptr(alpha), ptr(beta), ptr(y), a.numel(), C, act,
             current_stream())
    return y


def _act_bwd(dy, ref, act):
    dx = torch.empty_like(dy)
    lib.call(_k("nasseg_act_bwd", dy), ptr(dy), ptr(ref), ptr(dx), dy.numel(), act, current_stream())
    return dx


# ---------------------------------------------------------------------------
# depthwise convolution
# ---------------------------------------------------------------------------
class _DepthwiseConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride, pad, dil, relu_in):
        x = _cl(x)
        w = weight.contiguous()
        B, C, H, W = x.shape
        K = w.shape[-1]
        if w.shape[0] != C or w.shape[1] != 1 or w.shape[2] != K:
            raise NassegError("depthwise weight {} does not match C={}".format(tuple(w.shape), C))
        Ho, Wo = conv_out_size(H, K, stride, pad, dil), conv_out_size(W, K, stride, pad, dil)
        if Ho <= 0 or Wo <= 0:
            raise NassegError("depthwise conv output would be empty")
        s = current_stream()
        wt = _vec(x, K * K * C)
        lib.call("nasseg_dw_pack_weight", ptr(w), ptr(wt), C, K, 0, s)
        y = _new(x, B, C, Ho, Wo)
        lib.call(_k("nasseg_dwconv", x), ptr(x), ptr(wt), ptr(y), None, None, ACT_RELU if relu_in else ACT_NONE,
                 None, None, ACT_NONE, B, H, W, C, Ho, Wo, K, stride, pad, dil, 0, None, s)
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pad, dil, bool(relu_in))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, dil, relu_in = ctx.cfg
        dy = _cl(dy)
        B, C, H, W = x.shape
        K = w.shape[-1]
        Ho, Wo = dy.shape[2], dy.shape[3]
        s = current_stream()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = _vec(x, K * K * C)
            dx = _new(x, B, C, H, W)
            padb = dil * (K - 1) - pad
            if stride == 1 and padb >= 0:
                # correlation with the 180-degree rotated kernel
                lib.call("nasseg_dw_pack_weight", ptr(w), ptr(wt), C, K, 1, s)
                lib.call(_k("nasseg_dwconv", dy), ptr(dy), ptr(wt), ptr(dx), None, None, ACT_NONE, None, None,
                         ACT_NONE, B, Ho, Wo, C, H, W, K, 1, padb, dil, 0, None, s)
            else:
                lib.call("nasseg_dw_pack_weight", ptr(w), ptr(wt), C, K, 0, s)
                lib.call(_k("nasseg_dwconv", dy), ptr(dy), ptr(wt), ptr(dx), None, None, ACT_NONE, None, None,
                         ACT_NONE, B, Ho, Wo, C, H, W, K, stride, pad, dil, 1, None, s)
            if relu_in:
                dx = _act_bwd(dx, x, ACT_RELU)
        if ctx.needs_input_grad[1]:
            dw = _dw_wgrad(x, dy, w, None, None, ACT_RELU if relu_in else ACT_NONE,
                           (B, H, W, C, Ho, Wo, K, stride, pad, dil))
        return dx, dw, None, None, None, None


def depthwise_conv2d(x, weight, stride=1, padding=0, dilation=1, relu_in=False):
    """groups == channels convolution; ``relu_in`` fuses a preceding ReLU (DilConv)."""
    return _DepthwiseConv.apply(x, weight, int(stride), int(padding), int(dilation), bool(relu_in))


# ---------------------------------------------------------------------------
# dense convolution (1x1 and k x k) on the fp32 matrix cores
# ---------------------------------------------------------------------------
def _pack_dense(w, mode):
    """mode 'fwd' picks the layout nasseg_conv_fwd expects for this geometry; 1 = backward-data"""
    N, K, kh, kw = w.shape
    if mode == "fwd":
        mode = lib.query("nasseg_conv_fwd_pack_mode", K, kh, kw)
    if kh == 1 and kw == 1 and mode == 0:
        return w  # (N,K,1,1) contiguous already is [tap=0][N][K]
    wp = _vec(w, w.numel())
    lib.call("nasseg_conv_pack_weight", ptr(w), ptr(wp), N, K, kh, kw, mode, current_stream())
    return wp


_PACK_PLANS = {}
_PACK_SWEEP_AT = 1024  # plans; above it the entries of dead parameters are dropped


class _PackPlan(object):
    """Launch descriptor + destination buffer of one set of weights (see _pack_many).  `refs` are
    weak references to the source tensors: a plan whose parameters are gone is never served again
    (a new tensor may live at the same address) and is dropped at the next sweep."""
    __slots__ = ("n", "src", "dst", "dims", "views", "buf", "refs")

    def alive(self):
        return all(r() is not None for r in self.refs)


class PackMemo(list):
    """What ``packed_once`` remembers between the steps of ONE model / graphed stepper: the
    (key, plan) pairs of the chains seen last time - strong references, so the packed-weight
    buffers a captured hipGraph has baked in stay allocated for as long as their owner lives,
    whatever happens to the global cache - and the merged launch table built from them."""

    def __init__(self, *a):
        super(PackMemo, self).__init__(*a)
        self.merged = None


def _sweep_pack_plans():
    for k in [k for k, pl in _PACK_PLANS.items() if not pl.alive()]:
        del _PACK_PLANS[k]


class packed_once(object):
    """``with F.packed_once(memo): forward (+ backward) of one training step``

    Every conv chain re-packs its weights into the kernels' layouts with one small launch per
    chain and step (~50 launches on the headline network, each on the dependency path).  Within
    ONE step the parameters do not change, so inside this context the packs of all chains seen
    the last time ``memo`` (a ``PackMemo`` the caller keeps with the model) went through it are
    issued together at entry - nasseg_pack_weights takes any number of tensors - and the chains
    find their packed weights ready.  Chains met for the first time pack themselves as usual and
    are remembered in ``memo`` for the next entry.  Same kernel, same bytes: identical results.
    The context must not span a parameter update."""

    scope = None

    def __init__(self, memo):
        self.memo = memo

    def __enter__(self):
        self.prev, packed_once.scope = packed_once.scope, self
        self.done, self.seen, self.noted = set(), [], set()
        # only plans that still are the current ones of their keys (a plan rebuilt since has a
        # new buffer: whoever asks for that key will read the new one)
        entries = [(k, pl) for k, pl in self.memo if _PACK_PLANS.get(k) is pl]
        if entries:
            merged = getattr(self.memo, "merged", None)
            if merged is not None and (len(merged[4]) != len(entries)
                                       or any(a is not b[1] for a, b in zip(merged[4], entries))):
                merged = None
            if merged is None:
                plans = [pl for _, pl in entries]
                n = sum(pl.n for pl in plans)
                src = (ctypes.c_void_p * max(n, 1))()
                dst = (ctypes.c_void_p * max(n, 1))()
                dims = (ctypes.c_int * (7 * max(n, 1)))()
                j = 0
                for pl in plans:
                    for i in range(pl.n):
                        src[j], dst[j] = pl.src[i], pl.dst[i]
                        dims[7 * j:7 * j + 7] = pl.dims[7 * i:7 * i + 7]
                        j += 1
                merged = (n, src, dst, dims, plans)
                if isinstance(self.memo, PackMemo):
                    self.memo.merged = merged
            if merged[0]:
                lib.call("nasseg_pack_weights", merged[0], merged[1], merged[2], merged[3], current_stream())
            self.done.update(k for k, _ in entries)
        return self

    def __exit__(self, exc_type, exc, tb):
        packed_once.scope = self.prev
        if exc_type is None:
            self.memo[:] = self.seen
        return False


def _pack_many(like, items):
    """Re-pack several weights with ONE launch.  items: [(weight, kind)] or, for a slice of the
    input channels of a dense weight, [(weight, kind, koff, K)]; kind 'fwd' | 0 | 1 | 2 for dense
    weights (as _pack_dense; 5 = mode 1 with flipped taps, see _dense_backward_data), 'dw' |
    'dwflip' for depthwise ones.  Returns the packed tensors in order (the weight itself where
    its layout already is the packed one).

    The launch descriptor (pointer / shape tables) and the destination buffer of a given set of
    weights are built once and kept (_PackPlan): a chain packs the same parameters every step,
    and building the ctypes tables cost more host time than the launch.  The buffer is rewritten
    by every call; a forward's packed weights stay valid until the parameters change, i.e. for
    its own backward.  Plans are dropped only when their parameters are gone (never wholesale: a
    captured hipGraph holds their buffers' addresses - and, through its PackMemo, the plans)."""
    key = (like.device,) + tuple((it[0].data_ptr(), tuple(it[0].shape)) + tuple(it[1:]) for it in items)
    plan = _PACK_PLANS.get(key)
    if plan is not None and not plan.alive():
        plan = None  # (same addresses, other tensors: the old owner may still replay the old buffer)
    if plan is None:
        slots, descs, off = [], [], 0
        for item in items:
            w, kind = item[0], item[1]
            if kind in ("dw", "dwflip"):
                C, _, k, _ = w.shape
                d = (C, 1, k, k, 3 if kind == "dw" else 4, 0, 0)
                numel = w.numel()
            else:
                N, Ksrc, kh, kw = w.shape
                koff, K = (item[2], item[3]) if len(item) > 2 else (0, Ksrc)
                mode = lib.query("nasseg_conv_fwd_pack_mode", K, kh, kw) if kind == "fwd" else int(kind)
                if kh == 1 and kw == 1 and mode == 5:
                    mode = 1
                if kh == 1 and kw == 1 and mode == 0 and K == Ksrc:
                    slots.append(None)  # the weight itself
                    continue
                d = (N, K, kh, kw, mode, Ksrc if K != Ksrc else 0, koff)
                numel = N * K * kh * kw
            slots.append((off, numel))
            descs.append((w, d, off, numel))
            off += (numel + 3) // 4 * 4  # keep every packed tensor 16-byte aligned
        n = len(descs)
        plan = _PackPlan()
        plan.n = n
        plan.buf = _vec(like, off) if n else None
        plan.src = (ctypes.c_void_p * max(n, 1))(*[ptr(w) for w, _, _, _ in descs])
        plan.dst = (ctypes.c_void_p * max(n, 1))()
        plan.dims = (ctypes.c_int * (7 * max(n, 1)))()
        for j, (w, d, o, numel) in enumerate(descs):
            plan.dst[j] = ptr(plan.buf[o:o + numel])
            plan.dims[7 * j:7 * j + 7] = d
        plan.views = [None if sl is None else plan.buf[sl[0]:sl[0] + sl[1]] for sl in slots]
        plan.refs = [weakref.ref(it[0]) for it in items]
        if len(_PACK_PLANS) >= _PACK_SWEEP_AT:  # (parameters of discarded candidates)
            _sweep_pack_plans()
        _PACK_PLANS[key] = plan
        if packed_once.scope is not None:
            packed_once.scope.done.discard(key)  # (a new buffer: whatever was packed for this key is gone)
    scope = packed_once.scope
    if scope is not None and key not in scope.noted:
        scope.noted.add(key)
        scope.seen.append((key, plan))
    if plan.n and (scope is None or key not in scope.done):
        lib.call("nasseg_pack_weights", plan.n, plan.src, plan.dst, plan.dims, current_stream())
        if scope is not None:
            scope.done.add(key)  # (a weight used twice in the step is packed once)
    return [item[0] if v is None else v for item, v in zip(items, plan.views)]


def _dgrad_form(kh, kw, stride, pad, dil):
    """Backward-data of a stride-1 k x k conv is a forward conv over dy with flipped,
    role-swapped weights (pack kind 5) and pad' = dil*(k-1) - pad - the form the LDS-tiled
    3x3 kernel serves; everything else uses the transposed gather (pack kind 1)."""
    if stride == 1 and kh == kw and kh > 1 and dil * (kh - 1) - pad >= 0:
        return 5
    return 1


def _dense_dgrad_form(w, stride, pad, dil):
    """_dgrad_form for weight ``w`` (N,K,kh,kw); a forward conv over dy whose reduction
    axis (N) is so short that nasseg_conv_fwd would take its flat-packed path keeps the
    transposed form."""
    N, _, kh, kw = w.shape
    form = _dgrad_form(kh, kw, stride, pad, dil)
    if form == 5 and lib.query("nasseg_conv_fwd_pack_mode", N, kh, kw) != 0:
        return 1
    return form


def _dense_backward_data(dz, wb, form, x_shape, N, kh, kw, stride, pad, dil, res=None):
    """dx of a dense conv; wb packed with kind ``form`` (_dgrad_form); ``res`` (a map of dx's shape) is added in
    the epilogue."""
    B, K, H, W = x_shape
    Ho, Wo = dz.shape[2], dz.shape[3]
    dx = _new(dz, B, K, H, W)
    if form == 5:
        lib.call(_k("nasseg_conv_fwd", dz), ptr(dz), N, ptr(wb), ptr(dx), K, None, None, 0, None, None,
                 ACT_NONE, ptr(res), K if res is not None else 0, B, Ho, Wo, N, H, W, K, kh, kw, 1,
                 dil * (kh - 1) - pad, dil, 0, None, current_stream())
    else:
        lib.call(_k("nasseg_conv_fwd", dz), ptr(dz), N, ptr(wb), ptr(dx), K, None, None, 0, None, None,
                 ACT_NONE, ptr(res), K if res is not None else 0, B, Ho, Wo, N, H, W, K, kh, kw, stride, pad, dil, 1,
                 None, current_stream())
    return dx


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, dil):
        x = _cl(x)
        w = weight.contiguous()
        B, K, H, W = x.shape
        N, Kw, kh, kw = w.shape
        if Kw != K:
            raise NassegError("conv weight {} does not match C_in={}".format(tuple(w.shape), K))
        Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
        if Ho <= 0 or Wo <= 0:
            raise NassegError("conv output would be empty")
        y = _new(x, B, N, Ho, Wo)
        wp = _pack_dense(w, "fwd")
        lib.call(_k("nasseg_conv_fwd", x), ptr(x), K, ptr(wp), ptr(y), N, None, None, 0, None, ptr(bias),
                 ACT_NONE, None, 0, B, H, W, K, Ho, Wo, N, kh, kw, stride, pad, dil, 0, None,
                 current_stream())
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pad, dil, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, dil, has_bias = ctx.cfg
        dy = _cl(dy)
        B, K, H, W = x.shape
        N, _, kh, kw = w.shape
        Ho, Wo = dy.shape[2], dy.shape[3]
        s = current_stream()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            form = _dense_dgrad_form(w, stride, pad, dil)
            (wp,) = _pack_many(dy, [(w, form)])
            dx = _dense_backward_data(dy, wp, form, (B, K, H, W), N, kh, kw, stride, pad, dil)
        if ctx.needs_input_grad[1]:
            dw = _dense_wgrad(x, dy, w, None, None, ACT_NONE, (B, H, W, K, Ho, Wo, N, kh, kw, stride, pad, dil))
        if has_bias and ctx.needs_input_grad[2]:
            db = _colred(RED_SUM, dy, N, None, 0, None, 0, 1, B * Ho * Wo, N)
        return dx, dw, db, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1):
    """Dense convolution, groups == 1 (nn.Conv2d semantics, square stride/pad/dilation)."""
    return _Conv2d.apply(x, weight, bias, int(stride), int(padding), int(dilation))


# ---------------------------------------------------------------------------
# conv -> BN -> act chains with "normalise on read"
# ---------------------------------------------------------------------------
def _dw_backward_data(dz, wt, K, x_shape, stride, pad, dil, bn=None):
    """wt: the packed weight - flipped when the stride-1 correlation form applies, plain otherwise.
    bn = (z, scale, shift, mean, invstd, act) of the BatchNorm whose normalised output this conv
    read: the kernel then also masks the gradient with act' and emits the BatchNorm-backward
    partial sums.  Returns (dx, None | (rows buffer, number of rows))."""
    B, C, H, W = x_shape
    Ho, Wo = dz.shape[2], dz.shape[3]
    s = current_stream()
    dx = _new(dz, B, C, H, W)
    padb = dil * (K - 1) - pad
    if stride == 1 and padb >= 0:
        geom = (B, Ho, Wo, C, H, W, K, 1, padb, dil, 0)
    else:
        geom = (B, Ho, Wo, C, H, W, K, stride, pad, dil, 1)
    if bn is not None:
        nb = lib.query("nasseg_dwconv_bwd_data_bn_blocks", B, C, H, W, K, geom[7], geom[8], dil, geom[10])
        if nb > 0:
            z, scale, shift, mean, invstd, act = bn
            part = _rows_ws(dz, nb, C)
            lib.call(_k("nasseg_dwconv_bwd_data_bn", dz), ptr(dz), ptr(wt), ptr(dx), ptr(z), ptr(scale),
                     ptr(shift), ptr(mean), ptr(invstd), act, *geom, ptr(part), s)
            return dx, (part, nb)
    lib.call(_k("nasseg_dwconv", dz), ptr(dz), ptr(wt), ptr(dx), None, None, ACT_NONE, None, None,
             ACT_NONE, *geom, None, s)
    return dx, None


_IDENTITY = {}


def _identity_vectors(like, n):
    """(ones, zeros) of at least n floats on like's device - the "BatchNorm" that turns the fused
    backward-data epilogue into a plain act' mask (scale 1, shift 0, mean 0, invstd 1).  Created
    once per device and size class, never written."""
    key = (like.device, (n + 1023) // 1024)
    ent = _IDENTITY.get(key)
    if ent is None:
        m = key[1] * 1024
        ent = (torch.ones(m, device=like.device, dtype=torch.float32),
               torch.zeros(m, device=like.device, dtype=torch.float32))
        _IDENTITY[key] = ent
    return ent


# backward of pointwise conv + BatchNorm as one kernel where the chain allows it (csrc/conv_pwbwd.hip),
# for maps whose input + output exceed this many bytes (tools/kbench_pwbwd.py: 32 -> 32 at 4x128x256,
# 33 MB, one kernel 21 us / two kernels 26 us; 64 -> 64 at 4x32x64, 4 MB, 35 / 19 us - too few slabs)
FUSE_RES_GRAD = os.environ.get("NASSEG_FUSE_RES_GRAD", "1") != "0"  # (_ConvChain.backward: dx + dres in one epilogue)
FUSE_PW_BWD = os.environ.get("NASSEG_FUSE_PW_BWD", "1") != "0"
_PW_BWD_MIN_BYTES = int(os.environ.get("NASSEG_PW_BWD_MIN_BYTES", 24 << 20))
# the wide-input variant (K > 64: the four waves split N; round 3: chunks of the input and of the
# backward-data weight prefetched while the previous chunk is multiplied): 224 -> 64 at 4x256x512 (pre_clf,
# whose input gradient also carries the ReLU mask) 410-425 us against 710-730 us for the two kernels
# (tools/kbench_pwbwd.py), 192 -> 64 at 16x81x81 98 / 120 us, 192 -> 48 at 8x179x179 155 / 251 us; on maps
# too small for a slab per CU it loses (320 -> 64 at 16x11x11: 170 / 22 us), hence the pixel floor
_PW_BWD_WIDE = os.environ.get("NASSEG_PW_BWD_WIDE", "1") == "1"
_PW_BWD_WIDE_MIN_PIXELS = 1 << 16
# ConcatReduce's BatchNorm -> ReLU -> 1x1 conv on the concat slab as one node (the conv normalises on load)
FUSE_BN_RELU_CONV = os.environ.get("NASSEG_FUSE_BN_RELU_CONV", "1") != "0"
# Pool's 1x1 conv + BatchNorm -> 3x3 max pooling as one node (csrc/pool.hip: nasseg_maxpool_bn_fwd / _bwd)
FUSE_POOL_BN = os.environ.get("NASSEG_FUSE_POOL_BN", "1") != "0"
# ConcatReduce as one node fed by its producers' raw conv outputs (_CatReduce / Pending)
FUSE_CAT_REDUCE = os.environ.get("NASSEG_FUSE_CAT_REDUCE", "1") != "0"
# depthwise -> pointwise stages of a chain (SepConv, DilConv) as one kernel (csrc/sepconv.hip)
FUSE_SEPCONV = os.environ.get("NASSEG_FUSE_SEPCONV", "1") != "0"  # (the switch exists for A/B measurements)
# which pointwise forward / backward-data calls take the persistent kernel (include/nasseg.h:
# nasseg_conv_pw_min_pixels): unset = where it measured faster, 0 = wherever it can, a huge number = nowhere
_PW_MIN_PIXELS = os.environ.get("NASSEG_PW_MIN_PIXELS")
# ... and which take the N-split persistent kernel (nasseg_conv_pwn_mode): unset / 1 = where it measured faster,
# 0 = nowhere, 2 = wherever it can
_PWN_MODE = os.environ.get("NASSEG_PWN_MODE")


# elements of the stage's depthwise output above which a 5x5 stage runs as two kernels when the
# depthwise output has to be written anyway (training).  tools/kbench_sepconv.py on MI355X, fused
# vs separate in us: 32ch 128x256 21 / 29, 64ch 64x128 15 / 20, 64ch 128x256 46 / 48 - but
# 48ch 8x179x179 72 / 56, 24->64ch 256x512 93 / 79, 64ch dil-6 256x512 193 / 171: on large maps
# both forms are bandwidth-bound and the separate kernels keep more waves resident (the fused one
# holds the tile in LDS and its two phases do not overlap within a workgroup).  3x3 stages and
# inference (no depthwise output written) win at every size measured.
_SEPCONV_5X5_TRAIN_MAX = 10 << 20
# ... and, with 64 or more channels, already from 4 M elements (round 5, same table on MI355X: 64ch 128x256 45.1 / 42.6,
# 64ch 16x81x81 dilation 6 50.2 / 44.2 - but 64ch 64x128 14.5 / 19.6): the fused kernel's depthwise phase is bound by
# its vector-instruction issue (1721 VALU instructions per wave, tools/gpu.sh pmc), and the wider the tile's channel
# axis the fewer columns share a workgroup's weights
_SEPCONV_5X5_TRAIN_MAX_WIDE = 4 << 20


def _sepconv_ok(x, w_dw, w_pw, op_dw, op_pw, needs_grad):
    """Does nasseg_sepconv_fwd serve this depthwise conv (no BatchNorm behind it) followed by
    this pointwise conv - and is it the faster form here?"""
    B, C, H, W = x.shape
    k = w_dw.shape[-1]
    _, stride, pad, dil = op_dw[:4]
    N = w_pw.shape[0]
    if tuple(w_dw.shape) != (C, 1, k, k) or tuple(w_pw.shape) != (N, C, 1, 1):
        return False
    if op_pw[1:4] != (1, 0, 1):  # pointwise: stride 1, no padding
        return False
    Ho, Wo = conv_out_size(H, k, stride, pad, dil), conv_out_size(W, k, stride, pad, dil)
    if Ho <= 0 or Wo <= 0:
        return False
    limit = _SEPCONV_5X5_TRAIN_MAX_WIDE if (C >= 64 and needs_grad) else _SEPCONV_5X5_TRAIN_MAX
    if k == 5 and B * Ho * Wo * C > limit and (needs_grad or C % 16 != 0):
        return False
    return lib.query("nasseg_sepconv_blocks", B, C, Ho, Wo, N, k, stride, dil) > 0


# InvertedResidual's expansion never stored (csrc/irdw.hip; reference src/nn/layer_factory.py:125-158): a pointwise
# conv K -> N = 6 K + BatchNorm + activation in front of a 3x3 depthwise conv + BatchNorm, in a training step.  The
# expansion's statistics come from the moments of its INPUT (nasseg_irdw_stats), the depthwise forward and the
# one-kernel depthwise backward rebuild the expanded map on the matrix cores (nasseg_irdw_fwd / _bwd), the pointwise
# backward rebuilds it as it already did (nasseg_conv_pw_bwd_bn with z == NULL): the map - six times the block's input,
# 805 MB for 16 -> 96 at 4x512x1024 - is neither written nor read.  Where it pays (tools/kbench_irdw.py, MI355X, us for
# expansion + depthwise forward / depthwise backward): 16 -> 96 stride 2 at 4x512x1024 426 -> 230 / 404 -> 470,
# 24 -> 144 stride 1 at 4x256x512 257 -> 184 / 332 -> 318, 24 -> 144 stride 2 190 -> 135 / 164 -> 213 (level in time,
# taken for the bytes); not 32 -> 192 (no kernel of the pointwise backward rebuilds twelve channel tiles).  NASSEG_IRDW=0 switches it off (A/B); maps below NASSEG_IRDW_MIN_PIXELS keep the stored form (the
# extra launches of the statistics cost more than the bytes).
IRDW = os.environ.get("NASSEG_IRDW", "1") != "0"
_IRDW_MIN_PIXELS = int(os.environ.get("NASSEG_IRDW_MIN_PIXELS", 1 << 18))
# (stride 2 with K = 24: by the kernels alone the rebuilt backward loses what the forward wins - 190 -> 135 / 164 -> 213 us -
#  but replayed in lanes the step is level or ahead, 306.7 -> 308.5 images/s over three runs each, with 0.9 GB less HBM
#  traffic and 0.3 GiB less memory: profiles/r06_ab_irdw_s2_k24.txt)
_IRDW_S2_MAX_K = int(os.environ.get("NASSEG_IRDW_S2_MAX_K", 24))


def _irdw_ok(ops, i, weights, cur, pend, needs_in_grad, need_w, training):
    """op i is such an expansion, op i + 1 its depthwise conv, and every kernel involved serves the geometry"""
    if not IRDW or i + 1 >= len(ops):
        return False
    kind, stride, pad, dil, has_bn, act = ops[i][:6]
    kind2, stride2, pad2, dil2, has_bn2 = ops[i + 1][:5]
    w, w2 = weights[i], weights[i + 1]
    if not (kind == "dense" and kind2 == "dw" and has_bn and has_bn2 and training and ops[i + 1][6]):
        return False
    N, K, kh, kw = w.shape
    if not (kh == 1 and kw == 1 and stride == 1 and pad == 0 and w2.shape[-1] == 3 and pad2 == 1 and dil2 == 1
            and stride2 in (1, 2) and w2.shape[0] == N):
        return False
    if not (needs_in_grad and need_w):  # (the one-kernel backwards need both gradients)
        return False
    B, _, H, W = cur.shape
    if pend is not None and pend[0] is None and pend[1] is None and not pend[2]:
        return False
    return _irdw_geometry_ok(B, H, W, K, N, stride2)


def _irdw_geometry_ok(B, H, W, K, N, stride):
    """the part of _irdw_ok that is a function of the geometry alone: the form pays there AND every kernel involved
    exists - the forward drops z1 only where the expansion's backward has a kernel that rebuilds it (z == NULL)"""
    if B * H * W < _IRDW_MIN_PIXELS or not (N > K and K % 4 == 0):
        return False
    if not ((stride == 1 and N <= 144) or (stride == 2 and K <= _IRDW_S2_MAX_K)):
        return False
    return (lib.query("nasseg_irdw_config", B, H, W, K, N, stride, 0) > 0
            and lib.query("nasseg_irdw_config", B, H, W, K, N, stride, 1) > 0
            and lib.query("nasseg_conv_pw_bwd_kernel_id", B, H, W, K, N, 1) >= 0
            and lib.query("nasseg_dwconv_bwd_bn_rows", B, N, H, W, 3, stride, 1, 1) > 0)


# A chain's config (conv_chain): in_act0 = activation applied to the input on load, one _ChainOp per conv, the CALLER's
# grad mode, pool = (3, stride, 1) or None, defer = return the last BatchNorm unapplied (Pending), in_pact = activation
# of a Pending input (None: a plain one; else its statistics vector rides behind the per-op tensors)
_ChainCfg = collections.namedtuple("_ChainCfg", "in_act0 ops grad_mode pool defer in_pact")
_ChainOp = collections.namedtuple("_ChainOp", "kind stride pad dil has_bn act training momentum eps")
# What an op saves for backward: input x (read through the prologue psc, psh), raw conv output z, BatchNorm statistics,
# weight and the weight packed for backward-data; and, in ctx.meta, (form, prologue activation) with form: plain, the
# depthwise half of a SepConv stage, InvertedResidual's expansion never stored (z None) and the depthwise conv over it
_OpSaved = collections.namedtuple("_OpSaved", "x psc psh z stats w wb")
OP_PLAIN, OP_SEPCONV_DW, OP_IR_PW, OP_IR_DW = range(4)


class _ChainForward(object):
    """One chain's forward by the forms of DESIGN.md "Forward, per op": irdw, conv (or a SepConv stage), tail - each
    takes ``cur`` and its prologue ``pend`` = (scale, shift, act), returns the next and records one _OpSaved per op"""

    __slots__ = ("cfg", "prm", "w", "wp", "wb", "needs_grad", "saved", "meta", "s")

    def __init__(self, cfg, x, tensors, needs_grad, need_x):
        ops = cfg.ops
        self.cfg, self.needs_grad, self.s, self.saved, self.meta = cfg, needs_grad, current_stream(), [], []
        self.prm = [tensors[k:k + 6] for k in range(0, 6 * len(ops), 6)]  # (weight, gamma, beta, rm, rv, nbt)
        # every layout of every weight of the chain (forward now, backward-data later) is produced by one launch
        self.w = [p[0].contiguous() for p in self.prm]
        items = [(w, "dw" if op.kind == "dw" else "fwd") for op, w in zip(ops, self.w)]
        bwd_slot = [None] * len(ops)
        for i, (op, w) in enumerate(zip(ops, self.w)):
            if not needs_grad or (i == 0 and not need_x):
                continue
            if op.kind == "dw":
                if op.stride == 1 and op.dil * (w.shape[-1] - 1) - op.pad >= 0:
                    bwd_slot[i] = len(items)
                    items.append((w, "dwflip"))
                else:
                    bwd_slot[i] = i  # transposed gather reads the forward layout
            else:
                # (a chain whose producer is a BatchNorm uses the fused transposed kernel)
                fused = ((i > 0 and ops[i - 1].has_bn) or (i == 0 and cfg.in_act0)) and w.shape[1] % 4 == 0
                bwd_slot[i] = len(items)
                items.append((w, 1 if fused else _dense_dgrad_form(w, op.stride, op.pad, op.dil)))
        packed = _pack_many(x, items)
        self.wp = packed[:len(ops)]
        self.wb = [None if j is None else packed[j] for j in bwd_slot]

    def keep(self, i, form, x, pro, z, stats):
        """op i's record for backward; pro: the prologue (scale, shift, act) its input was read through, or None"""
        if self.needs_grad:
            psc, psh, pact = pro if pro is not None else (None, None, ACT_NONE)
            self.saved.append(_OpSaved(x, psc, psh, z, stats, self.w[i], self.wb[i]))
            self.meta.append((form, pact))

    def irdw(self, i, cur, pend):
        """ops i, i + 1: InvertedResidual's pointwise expansion + BatchNorm + activation and its 3x3 depthwise conv +
        BatchNorm with the expanded map never stored (csrc/irdw.hip).  Returns (cur, pend, stats) after op i + 1."""
        op, op2 = self.cfg.ops[i], self.cfg.ops[i + 1]
        _, gamma, beta, rm, rv, nbt = self.prm[i]
        w = self.w[i]
        B, K, H, W = cur.shape
        N = w.shape[0]
        psc, psh, pact = pend if pend is not None else (None, None, ACT_NONE)
        st1 = _vec(cur, 4 * N)
        mean1, invstd1, scale1, shift1 = _bn_parts(st1, N)
        wsm = _ws(cur, lib.query("nasseg_irdw_stats_workspace", K))
        lib.call(_k("nasseg_irdw_stats", cur), ptr(cur), ptr(w), ptr(psc), ptr(psh), pact, B, H, W, K, N,
                 float(op.eps), float(op.momentum), ptr(gamma), ptr(beta), ptr(mean1), ptr(invstd1), ptr(scale1),
                 ptr(shift1), ptr(rm), ptr(rv), ptr(nbt), ptr(wsm), self.s)
        self.keep(i, OP_IR_PW, cur, pend, None, st1)
        Ho, Wo = conv_out_size(H, 3, op2.stride, 1, 1), conv_out_size(W, 3, op2.stride, 1, 1)
        z2 = _new(cur, B, N, Ho, Wo)
        rows2 = lib.query("nasseg_irdw_rows", B, H, W, K, N, op2.stride, 0)
        part2 = _rows_ws(cur, rows2, N)
        lib.call(_k("nasseg_irdw_fwd", cur), ptr(cur), ptr(w), ptr(self.wp[i + 1]), ptr(z2), ptr(psc), ptr(psh),
                 pact, ptr(scale1), ptr(shift1), op.act, B, H, W, K, N, Ho, Wo, op2.stride, ptr(part2), self.s)
        st2, _, _, scale2, shift2 = _bn_head(cur, N, B * Ho * Wo, z2.shape, self.prm[i + 1][1:], op2.training,
                                             op2.momentum, op2.eps, rows=(part2, rows2))
        # (its input None: the depthwise conv's input does not exist - backward rebuilds it from op i's)
        self.keep(i + 1, OP_IR_DW, None, (scale1, shift1, op.act), z2, st2)
        return z2, (scale2, shift2, op2.act), st2

    def conv(self, i, cur, pend, res, stage=None):
        """op i with its BatchNorm statistics, eval parameters or folded epilogue (which consumes res) - or, stage =
        i - 1, a SepConv stage's pointwise half (csrc/sepconv.hip; cur, pend: the depthwise half's).
        Returns cur, pend, stats, res."""
        op, w = self.cfg.ops[i], self.w[i]
        B, K, H, W = cur.shape
        last = i == len(self.cfg.ops) - 1
        dpend = None
        if stage is not None:  # (geometry of the stage's depthwise output; the prologue belongs to that half)
            dop, dk = self.cfg.ops[stage], self.w[stage].shape[-1]
            H, W = (conv_out_size(d, dk, dop.stride, dop.pad, dop.dil) for d in (H, W))
            dpend, pend = pend, None
        if op.kind == "dw":  # (pro_ok: the kernel applies pend as it loads; stats_ok: its epilogue emits statistics)
            N, kh, kw = K, w.shape[-1], w.shape[-1]
            if w.shape[0] != K or w.shape[1] != 1:
                raise NassegError("depthwise weight {} does not match C={}".format(tuple(w.shape), K))
            stats_ok = bool(lib.query("nasseg_dwconv_strip_ok", kh, op.stride, op.dil))
            pro_ok = stats_ok or (pend is not None and pend[0] is None and pend[2] == ACT_RELU)
        else:
            N, Kw, kh, kw = w.shape
            if Kw != K:
                raise NassegError("conv weight {} does not match C_in={}".format(tuple(w.shape), K))
            pro_ok = kh == 1 and kw == 1 and op.stride == 1 and op.pad == 0 and K % 4 == 0 and N % 4 == 0
            stats_ok = N % 4 == 0
        Ho, Wo = conv_out_size(H, kh, op.stride, op.pad, op.dil), conv_out_size(W, kw, op.stride, op.pad, op.dil)
        if Ho <= 0 or Wo <= 0:
            raise NassegError("conv output would be empty")
        if pend is not None and not pro_ok:
            cur = (_affine_act(cur, pend[0], pend[1], None, pend[2]) if pend[0] is not None
                   else _axpby(cur, None, None, None, pend[2]))
            pend = None
        psc, psh, pact = pend if pend is not None else (None, None, ACT_NONE)
        M = B * Ho * Wo
        z = _new(cur, B, N, Ho, Wo)
        fold = (op.has_bn and not op.training and not self.needs_grad
                and not (op.kind == "dw" and last and res is not None))
        stats, part, nblk = None, None, 0
        if op.has_bn:  # (eval parameters before the conv, whose epilogue may fold them; statistics after it)
            stats, parts = _bn_alloc(cur, N, op.training, M, z.shape)
            scale, shift = parts[2:]
            if not op.training:
                _bn_fill(parts, N, M, self.prm[i][1:], False, op.momentum, op.eps)
            elif stats_ok:
                if stage is not None:
                    nblk = lib.query("nasseg_sepconv_blocks", B, K, Ho, Wo, N, dk, dop.stride, dop.dil)
                elif op.kind == "dw":
                    nblk = lib.query("nasseg_dwconv_stats_blocks", B, N, Ho, Wo, kh, op.stride, op.dil)
                else:
                    nblk = lib.query("nasseg_conv_fwd_stats_rows", B, Ho, Wo, N, K, kh, kw, op.stride, op.pad, op.dil)
                part = _rows_ws(cur, nblk, N)
        # inference: BatchNorm (+ act, + residual) folded into the conv's epilogue
        o_sc, o_sh, o_act = (scale, shift, op.act) if fold else (None, None, ACT_NONE)
        o_res = res if (fold and last) else None
        if stage is not None:
            zdw = _new(cur, B, K, Ho, Wo) if self.needs_grad else None
            dsc, dsh, dact = dpend if dpend is not None else (None, None, ACT_NONE)
            lib.call(_k("nasseg_sepconv_fwd", cur), ptr(cur), ptr(self.wp[stage]), ptr(w), ptr(zdw), ptr(z), ptr(dsc),
                     ptr(dsh), dact, ptr(o_sc), ptr(o_sh), o_act, B, cur.shape[2], cur.shape[3], K, Ho, Wo, N,
                     dk, dop.stride, dop.pad, dop.dil, ptr(part), self.s)
            self.keep(stage, OP_SEPCONV_DW, cur, dpend, zdw, None)
            cur = zdw
        elif op.kind == "dw":
            lib.call(_k("nasseg_dwconv", cur), ptr(cur), ptr(self.wp[i]), ptr(z), ptr(psc), ptr(psh), pact, ptr(o_sc),
                     ptr(o_sh), o_act, B, H, W, K, Ho, Wo, kh, op.stride, op.pad, op.dil, 0, ptr(part), self.s)
        else:
            lib.call(_k("nasseg_conv_fwd", cur), ptr(cur), K, ptr(self.wp[i]), ptr(z), N, ptr(psc), ptr(psh), pact,
                     ptr(o_sc), ptr(o_sh), o_act, ptr(o_res), N, B, H, W, K, Ho, Wo, N, kh, kw,
                     op.stride, op.pad, op.dil, 0, ptr(part), self.s)
        self.keep(i, OP_PLAIN, cur, pend, z, stats)
        if fold or not op.has_bn:
            return z, None, stats, (None if (fold and last) else res)
        if op.training:
            _bn_fill(parts, N, M, self.prm[i][1:], True, op.momentum, op.eps, z,
                     (part, nblk) if part is not None else None)
        return z, (scale, shift, op.act), stats, res

    def tail(self, cur, pend, stats, res):
        """(y, statistics of a deferred tail, pooling indices, pooling applied the BatchNorm).  Pool (layer_factory.py:
        161-178): 3x3 max pooling applies a pending last BatchNorm as it loads the raw conv output."""
        if self.cfg.pool is None:
            if pend is None:
                return (_axpby(cur, res, None, None) if res is not None else cur), None, None, False
            if self.cfg.defer and res is None and pend[0] is not None:
                # deferred tail: the consumer applies act(scale*z + shift) as it loads (Pending below); what
                # comes back in backward is still the gradient w.r.t. the BatchNorm's activated output
                return cur, stats, None, False
            return _affine_act(cur, pend[0], pend[1], res, pend[2]), None, None, False
        pk, ps, pp = self.cfg.pool
        B, N, Hc, Wc = cur.shape
        Hp, Wp = conv_out_size(Hc, pk, ps, pp, 1), conv_out_size(Wc, pk, ps, pp, 1)
        if Hp <= 0 or Wp <= 0:
            raise NassegError("max pooling output would be empty")
        psc, psh = (pend[0], pend[1]) if pend is not None else (None, None)
        if (res is not None or (pend is not None and pend[2] != ACT_NONE) or pk != 3 or pp != 1
                or ps not in (1, 2)):
            raise NassegError("conv_chain: the pooled tail serves conv + BatchNorm -> 3x3 max pooling only")
        y = _new(cur, B, N, Hp, Wp)
        pool_idx = torch.empty((B, Hp, Wp, N), device=cur.device, dtype=torch.uint8) if self.needs_grad else None
        lib.call(_k("nasseg_maxpool_bn_fwd", cur), ptr(cur), ptr(psc), ptr(psh), ptr(y), ptr(pool_idx), B, Hc,
                 Wc, N, Hp, Wp, ps, pp, self.s)
        return y, None, pool_idx, pend is not None


# From op i's backward to op i - 1's: gradient g w.r.t. op i - 1's output, the rows of its BatchNorm-backward sums if
# the kernel that made g emitted them, masked = g carries its act', dres = the residual's gradient still to return
# (None once an epilogue added it into dx), in_masked = dx carries in_act0'.  _BnBwd: act = the mask g still lacks.
_Flow = collections.namedtuple("_Flow", "g rows masked dres in_masked")
_BnBwd = collections.namedtuple("_BnBwd", "scale shift mean invstd sums training act")
# The forms of an op's backward, DESIGN.md "Backward, per op" (in its order of precedence)
BWD_IRDW, BWD_DW_BN, BWD_FLAT_BN, BWD_PW_BN, BWD_WGRAD_BN, BWD_APPLY = range(6)


class _ChainBackward(collections.namedtuple("_ChainBackward", "ops recs meta need in_act0 fuse_res s")):
    """One chain's backward, op by op (op): plan picks the form, bn_head runs the BatchNorm backward, then irdw, dw_bn,
    flat_bn, pw_bn or generic take the _Flow from op i + 1 and return (weight gradient, _Flow for op i - 1)"""

    def plan(self, i, need_dw, need_dx):
        """(form, its rows or slabs) of op i, which has a BatchNorm"""
        op, r, (form, pact) = self.ops[i], self.recs[i], self.meta[i]
        if form == OP_IR_DW:
            return BWD_IRDW, 1
        if form == OP_IR_PW:  # (the pointwise backward rebuilds the expansion it never stored: z == NULL)
            B, K, H, W = r.x.shape
            return BWD_PW_BN, lib.query("nasseg_conv_pw_bwd_slabs", B, H, W, K, r.w.shape[0])
        nsl = _pw_bwd_slabs(op.kind, r.x, r.z, r.w, op.stride, op.pad, need_dw, need_dx, i, self.ops)
        if nsl > 0:
            return BWD_PW_BN, nsl
        rows = _dw_bwd_rows(op.kind, r.x, r.z, r.w, op.stride, op.pad, op.dil, need_dw, need_dx, i, self.ops)
        if rows > 0:
            return BWD_DW_BN, rows
        if _flat_bn_ok(op.kind, need_dw, need_dx, r.psc, r.psh, pact, r.w, r.w.shape[0], r.z):
            return BWD_FLAT_BN, 0
        if need_dw and _wgrad_bn_ok(op.kind, r.x, r.z, r.w, op.stride, op.pad, op.dil):
            return BWD_WGRAD_BN, 0
        return BWD_APPLY, 0

    def bn_head(self, i, fl, plan):
        """op i's BatchNorm backward sums (from the rows that came with g, or reduced) and, BWD_APPLY, dz: returns
        (_BnBwd, dz, dgamma, dbeta)"""
        op, r = self.ops[i], self.recs[i]
        N = r.w.shape[0]
        M = r.x.shape[0] * r.x.shape[2] * r.x.shape[3] if r.z is None else r.z.shape[0] * r.z.shape[2] * r.z.shape[3]
        mean, invstd, scale, shift = _bn_parts(r.stats, N)
        sums = _vec(fl.g, 2 * N)
        act_left = ACT_NONE if (fl.rows is not None or fl.masked) else op.act  # (the mask still to be applied to g)
        # g arrived masked with its per-workgroup {sum g, sum g*xhat} rows: few enough for the apply kernel to add
        # them up itself (lazy_rows), or summed here - else the sums by a reduction (or its rows, for the apply)
        lazy_rows = fl.rows if (fl.rows is not None and plan == BWD_APPLY and _rows_small(fl.rows[1], N)) else None
        if fl.rows is not None and lazy_rows is None:
            lib.call("nasseg_rows_sum", ptr(fl.rows[0]), fl.rows[1], 2 * N, ptr(sums), self.s)
        elif fl.rows is None:
            lazy_rows = _bn_bwd_reduce(fl.g, r.z, scale, shift, mean, invstd, act_left, sums, M, N, plan == BWD_APPLY)
        dgamma = sums[N:2 * N] if self.need[3 + 6 * i + 1] else None
        dbeta = sums[0:N] if self.need[3 + 6 * i + 2] else None
        dz = None
        if plan == BWD_APPLY:
            dz = _bn_bwd_apply(fl.g, r.z, scale, shift, mean, invstd, sums, M, N, op.training, act_left,
                               torch.empty_like(r.z), lazy_rows)
        return _BnBwd(scale, shift, mean, invstd, sums, op.training, act_left), dz, dgamma, dbeta

    def producer_bn(self, i, K):
        """(z, scale, shift, mean, invstd, act) of the chain's BatchNorm that produced op i's input, for the epilogue of
        op i's backward-data - at op 0 after an activation on load (DilConv, pre_clf) an identity BatchNorm: act'"""
        if i > 0 and self.ops[i - 1].has_bn and K % 4 == 0:
            p = self.recs[i - 1]
            mean, invstd, scale, shift = _bn_parts(p.stats, K)
            return p.z, scale, shift, mean, invstd, self.ops[i - 1].act
        if i == 0 and self.in_act0 and K % 4 == 0:
            x = self.recs[0].x
            if self.ops[0].kind == "dw":
                one, zero = _identity_vectors(x, K)
                return x, one, zero, zero, one, self.in_act0
            return x, None, None, None, None, self.in_act0  # mask-only epilogue
        return None

    def irdw(self, i, fl, bn):
        """the 3x3 depthwise conv behind a rebuilt expansion: nasseg_irdw_bwd with z1 = W1 x from op i - 1"""
        op, r = self.ops[i], self.recs[i]
        x_in, xpsc, xpsh, _, st1, w1, _ = self.recs[i - 1]
        Bc, K1, H, W = x_in.shape
        _, K, Ho, Wo = r.z.shape
        mean1, invstd1, scale1, shift1 = _bn_parts(st1, K)
        rows = lib.query("nasseg_irdw_rows", Bc, H, W, K1, K, op.stride, 1)
        dwt = torch.empty_like(r.w)
        ws = _ws(fl.g, rows * 9 * K)
        part = _rows_ws(fl.g, rows, K)
        g_in = _new(fl.g, Bc, K, H, W)
        lib.call(_k("nasseg_irdw_bwd", x_in), ptr(x_in), ptr(w1), ptr(fl.g), ptr(r.z), ptr(r.wb), int(op.stride == 1),
                 ptr(g_in), _finish_wgrad(ws, dwt, 9, K, 1, 0), ptr(ws), ptr(xpsc), ptr(xpsh), self.meta[i - 1][1],
                 ptr(scale1), ptr(shift1), ptr(mean1), ptr(invstd1), self.ops[i - 1].act,
                 ptr(bn.scale), ptr(bn.shift), ptr(bn.mean), ptr(bn.invstd), ptr(bn.sums), int(bn.training), bn.act,
                 Bc, H, W, K1, K, Ho, Wo, op.stride, ptr(part), self.s)
        return dwt, _Flow(g_in, (part, rows), False, fl.dres, fl.in_masked)

    def dw_bn(self, i, fl, bn, rows):
        """3x3 depthwise conv between two BatchNorms of the chain, its whole backward in one pass (csrc/dwconv.hip):
        BatchNorm backward on load, weight gradient, masked input gradient + the sums of the BatchNorm in front"""
        op, r = self.ops[i], self.recs[i]
        Bc, K, H, W = r.x.shape
        _, _, Ho, Wo = r.z.shape
        zp, psc_, psh_, pmu_, pis_, pact_ = self.producer_bn(i, K)
        dwt = torch.empty_like(r.w)
        ws = _ws(r.x, rows * 9 * K)
        part = _rows_ws(r.x, rows, K)
        g_in = _new(r.x, Bc, K, H, W)
        lib.call(_k("nasseg_dwconv_bwd_bn", r.x), ptr(r.x), ptr(fl.g), ptr(r.z), ptr(r.wb), int(op.stride == 1),
                 ptr(g_in), _finish_wgrad(ws, dwt, 9, K, 1, 0), ptr(ws), ptr(psc_), ptr(psh_), ptr(pmu_),
                 ptr(pis_), pact_, ptr(bn.scale), ptr(bn.shift), ptr(bn.mean), ptr(bn.invstd), ptr(bn.sums),
                 int(bn.training), bn.act, Bc, H, W, K, Ho, Wo, 3, op.stride, op.pad, op.dil, ptr(part), self.s)
        return dwt, _Flow(g_in, (part, rows), False, fl.dres, fl.in_masked)

    def flat_bn(self, i, fl, bn):
        """the stem (small-K k x k conv, no gradient for the image): BatchNorm backward on load in the
        weight-gradient kernel, dz never written (nasseg_conv_wgrad_bn_flat)"""
        op, r = self.ops[i], self.recs[i]
        Bc, K, H, W = r.x.shape
        N, _, kh, kw = r.w.shape
        _, _, Ho, Wo = r.z.shape
        dwt = torch.empty_like(r.w)
        ws = _ws(r.x, lib.query("nasseg_conv_wgrad_workspace", Bc, Ho, Wo, N, K, kh, kw))
        lib.call(_k("nasseg_conv_wgrad_bn_flat", r.x), ptr(r.x), K, ptr(fl.g), N, ptr(r.z), N,
                 _finish_wgrad(ws, dwt, kh * kw, N, K, 1), ptr(ws), ptr(bn.scale), ptr(bn.shift), ptr(bn.mean),
                 ptr(bn.invstd), ptr(bn.sums), int(bn.training), bn.act, Bc, H, W, K, Ho, Wo, N, kh, kw,
                 op.stride, op.pad, op.dil, self.s)
        return dwt, _Flow(None, None, False, fl.dres, fl.in_masked)

    def pw_bn(self, i, fl, bn, nsl):
        """pointwise conv + BatchNorm in ONE kernel, dz never written (csrc/conv_pwbwd.hip).  Op 0 after an activation
        on load, or a widening conv behind a BatchNorm of the chain (_pw_bwd_slabs): dx is masked with act' from the
        ACTIVATED input tile and, K <= 64, comes with the per-slab sums of that BatchNorm's backward (dx_stats)."""
        r, pact = self.recs[i], self.meta[i][1]
        Bc, K, H, W = r.x.shape
        N = r.w.shape[0]
        dwt = torch.empty_like(r.w)
        ws = _ws(r.x, nsl * N * K)
        g_in = _new(r.x, Bc, K, H, W)
        behind_bn = i > 0 and self.ops[i - 1].has_bn
        dx_act = pact if ((i == 0 and self.in_act0 and r.psc is None and r.psh is None) or behind_bn) else ACT_NONE
        part = pmu_ = pis_ = None
        skip_g = fl.dres if (self.fuse_res and i == 0 and K % 4 == 0) else None  # (x is also the block's skip)
        if behind_bn and K <= 64:
            pmu_, pis_ = _bn_parts(self.recs[i - 1].stats, K)[:2]
            part = _rows_ws(r.x, nsl, K)
        # (z only where the kernel loads it: where it rebuilds z = W x the argument is NULL - an explicit
        #  contract instead of a pointer the kernel ignores, and NULL is also what says "never stored")
        z_arg = r.z if (r.z is not None and lib.query("nasseg_conv_pw_bwd_reads_z", Bc, H, W, K, N)) else None
        lib.call(_k("nasseg_conv_pw_bwd_bn", r.x), ptr(r.x), ptr(fl.g), ptr(z_arg), ptr(r.wb), ptr(g_in),
                 _finish_wgrad(ws, dwt, 1, N, K, 0), ptr(ws), ptr(r.psc), ptr(r.psh), pact, dx_act,
                 ptr(bn.scale), ptr(bn.shift), ptr(bn.mean), ptr(bn.invstd), ptr(bn.sums), int(bn.training), bn.act,
                 Bc, H, W, K, N, ptr(pmu_), ptr(pis_), ptr(part), ptr(skip_g), self.s)
        return dwt, _Flow(g_in, (part, nsl) if part is not None else None, behind_bn,
                          fl.dres if skip_g is None else None, bool(dx_act) and i == 0)

    def generic(self, i, fl, bn, dz, need_dw, need_dx):
        """a depthwise or dense conv: weight gradient (bn given: with the BatchNorm backward on load, which leaves dz)
        and backward-data with the producer's BatchNorm in its epilogue - or, op 0, the residual's gradient"""
        op, r, pact = self.ops[i], self.recs[i], self.meta[i][1]
        Bc, K, H, W = r.x.shape
        _, N, Ho, Wo = r.z.shape
        kh, kw = r.w.shape[2], r.w.shape[3]
        bn_prev = self.producer_bn(i, K) if need_dx else None
        dw = op.kind == "dw"
        geom = ((Bc, H, W, K, Ho, Wo, kh, op.stride, op.pad, op.dil) if dw
                else (Bc, H, W, K, Ho, Wo, N, kh, kw, op.stride, op.pad, op.dil))
        dwt = None
        if bn is not None:
            dwt, dz = _wgrad_bn(op.kind, r.x, fl.g, r.z, r.w, r.psc, r.psh, pact, bn, geom if dw else (Bc, H, W, K, N))
        elif need_dw:
            dwt = (_dw_wgrad if dw else _dense_wgrad)(r.x, dz, r.w, r.psc, r.psh, pact, geom)
        if not need_dx:
            return dwt, _Flow(None, None, False, fl.dres, fl.in_masked)
        if dw:
            g, rows = _dw_backward_data(dz, r.wb, kh, (Bc, K, H, W), op.stride, op.pad, op.dil, bn_prev)
            return dwt, _Flow(g, rows, False, fl.dres, fl.in_masked)
        if bn_prev is not None:
            g = _new(r.x, Bc, K, H, W)
            zp, psc_, psh_, pmu_, pis_, pact_ = bn_prev
            pw1 = kh == 1 and kw == 1 and op.stride == 1 and op.pad == 0
            nb = lib.query("nasseg_conv_fwd_stats_blocks", Bc, H, W, K, N, 2 * int(pw1)) if pmu_ is not None else 0
            part = _rows_ws(r.x, nb, K) if nb else None
            lib.call(_k("nasseg_conv_bwd_data_bn", dz), ptr(dz), N, ptr(r.wb), ptr(g), K, ptr(zp), K,
                     ptr(psc_), ptr(psh_), ptr(pmu_), ptr(pis_), pact_, Bc, Ho, Wo, N, H, W,
                     K, kh, kw, op.stride, op.pad, op.dil, ptr(part), self.s)
            return dwt, _Flow(g, (part, nb), False, fl.dres, fl.in_masked)
        res = fl.dres if (self.fuse_res and i == 0) else None  # (added in the epilogue: it is inside dx)
        g = _dense_backward_data(dz, r.wb, _dense_dgrad_form(r.w, op.stride, op.pad, op.dil), (Bc, K, H, W), N, kh,
                                 kw, op.stride, op.pad, op.dil, res)
        return dwt, _Flow(g, None, False, fl.dres if res is None else None, fl.in_masked)

    def op(self, i, fl):
        """op i's backward: ((dw, dgamma, dbeta), _Flow for op i - 1); its g None ends the chain's backward"""
        need_dw, need_dx = self.need[3 + 6 * i], i > 0 or self.need[1]
        go_on = need_dw or need_dx
        bn, dz, dgamma, dbeta, plan, n = None, fl.g, None, None, BWD_APPLY, 0
        if self.ops[i].has_bn:
            plan, n = self.plan(i, need_dw, need_dx) if go_on else (None, 0)
            bn, dz, dgamma, dbeta = self.bn_head(i, fl, plan)
        if not go_on:
            return (None, dgamma, dbeta), fl._replace(g=None)
        if plan == BWD_IRDW:
            dwt, fl = self.irdw(i, fl, bn)
        elif plan == BWD_DW_BN:
            dwt, fl = self.dw_bn(i, fl, bn, n)
        elif plan == BWD_FLAT_BN:
            dwt, fl = self.flat_bn(i, fl, bn)
        elif plan == BWD_PW_BN:
            dwt, fl = self.pw_bn(i, fl, bn, n)
        else:
            dwt, fl = self.generic(i, fl, bn if plan == BWD_WGRAD_BN else None, dz, need_dw, need_dx)
        return (dwt, dgamma, dbeta), fl


class _ConvChain(torch.autograd.Function):
    """A run of convolutions (dense on the MFMA path or depthwise), each optionally followed
    by BatchNorm (+ReLU/ReLU6), as ONE autograd node in which a normalised activation that
    only feeds the next convolution is never written: the producer emits the raw conv output
    z plus the BatchNorm statistics (epilogue), the consumer applies act(scale*z + shift) as
    it loads its operand (prologue), backward recomputes the same on load.  Only the chain's
    final output is materialised (with the block's residual add fused in).  cfg: a _ChainCfg;
    tensors: per op (weight, gamma, beta, running_mean, running_var, num_batches_tracked), None
    where absent, then the statistics vector of a Pending input (or None)."""

    @staticmethod
    def forward(ctx, cfg, x, residual, *tensors):
        res_is_x = residual is not None and residual is x  # (InvertedResidual: the block's input is its skip)
        x = _cl(x)
        # the statistics vector a deferred tail hands out never has a gradient: without this autograd would
        # materialise a zero "gradient" for it in every backward (one fill launch per chain and step)
        ctx.set_materialize_grads(False)
        # (under no_grad ctx.needs_input_grad still reports the parameters' requires_grad flags: nothing
        #  will ever call backward then, and inference may fold every BatchNorm into its conv's epilogue)
        needs_grad = cfg.grad_mode and any(ctx.needs_input_grad)
        res = _cl(residual) if residual is not None else None
        pend = (None, None, cfg.in_act0) if cfg.in_act0 else None
        if cfg.in_pact is not None:
            # the input is another chain's Pending: its BatchNorm + activation are op 0's prologue; backward returns
            # the gradient w.r.t. the ACTIVATED input - exactly what a plain backward-data of op 0 computes
            pend = _scale_shift(tensors[-1], x.shape[1]) + (cfg.in_pact,)
        f = _ChainForward(cfg, x, tensors, needs_grad, ctx.needs_input_grad[1])
        ops, n = cfg.ops, len(cfg.ops)
        cur, stats, i = x, None, 0
        while i < n:
            if (needs_grad and i + 1 < n
                    and _irdw_ok(ops, i, f.w, cur, pend, i > 0 or ctx.needs_input_grad[1],
                                 ctx.needs_input_grad[3 + 6 * i] and ctx.needs_input_grad[3 + 6 * (i + 1)],
                                 ops[i].training)):
                cur, pend, stats = f.irdw(i, cur, pend)
                i += 2
            elif (ops[i].kind == "dw" and not ops[i].has_bn and i + 1 < n and FUSE_SEPCONV
                  and ops[i + 1].kind == "dense" and not (i + 2 == n and res is not None and not needs_grad)
                  and _sepconv_ok(cur, f.w[i], f.w[i + 1], ops[i], ops[i + 1], needs_grad)):
                # SepConv / DilConv stage: this depthwise conv and the pointwise conv i + 1 as ONE kernel
                cur, pend, stats, res = f.conv(i + 1, cur, pend, res, stage=i)
                i += 2
            else:
                cur, pend, stats, res = f.conv(i, cur, pend, res)
                i += 1
        y, tail, pool_idx, pool_fused = f.tail(cur, pend, stats, res)
        if needs_grad:
            ctx.save_for_backward(*[t for rec in f.saved for t in rec] + ([pool_idx] if cfg.pool is not None else []))
            ctx.meta = (cfg, f.meta, residual is not None, res_is_x, pool_fused)
            ctx.n_inputs = 3 + len(tensors)
        if not cfg.defer:
            return y
        if tail is not None:
            ctx.mark_non_differentiable(tail)
        return y, tail  # (mean | invstd | scale | shift of the last BatchNorm, or None)

    @staticmethod
    def backward(ctx, dy, *_unused):
        if dy is None:  # (no gradient reaches the chain's output: nothing to hand on)
            return (None,) * ctx.n_inputs
        cfg, meta, has_res, res_is_x, pool_fused = ctx.meta
        n = len(cfg.ops)
        sv, k = ctx.saved_tensors, len(_OpSaved._fields)
        recs = [_OpSaved._make(sv[j:j + k]) for j in range(0, k * n, k)]
        need = ctx.needs_input_grad
        g = _cl(dy)
        dres = g if (has_res and need[2]) else None
        # x is also the residual: both gradients go to the same tensor, and autograd would add them with a launch of
        # its own - where op 0's input gradient comes from the plain backward-data call, its epilogue adds dres
        fuse_res = FUSE_RES_GRAD and res_is_x and dres is not None and need[1] and not cfg.in_act0
        fl = _Flow(g, None, False, dres, False)
        if cfg.pool is not None:
            fl = _pool_backward(cfg.pool, fl, recs[-1], sv[k * n], pool_fused)
        elif _TAIL_ROWS:
            # a consumer of this chain's deferred tail (_CatReduce, a junction, ...) has already masked the gradient
            # and summed it against the last BatchNorm's xhat: its rows come by the side of the gradient tensor
            rows = _take_tail_rows(dy)
            fl = fl._replace(rows=rows if cfg.ops[-1].has_bn else None)
        chain = _ChainBackward(cfg.ops, recs, meta, need, cfg.in_act0, fuse_res, current_stream())
        grads = [None] * (6 * n)
        for i in range(n - 1, -1, -1):
            grads[6 * i:6 * i + 3], fl = chain.op(i, fl)
            if fl.g is None:
                break
        dx = None
        if fl.g is not None and need[1]:
            dx = fl.g
            if cfg.in_act0 and fl.rows is None and not fl.in_masked:
                # the chain started with an activation applied on load and the backward-data
                # kernel had no fused mask for this geometry
                dx = _act_bwd(dx, recs[0].x, cfg.in_act0)
        return (None, dx, fl.dres) + tuple(grads) + (None,)


def _pool_backward(pool, fl, last, pool_idx, pool_fused):
    """the pooled tail: gradient w.r.t. the last BatchNorm's output by a gather over the windows - together with
    that BatchNorm's backward sums when the pooling had applied it on load"""
    (pk, ps, pp), g, s = pool, fl.g, current_stream()
    Bp, Np, Hz, Wz = last.z.shape
    g_full = _new(g, Bp, Np, Hz, Wz)
    nb = lib.query("nasseg_maxpool_bn_bwd_blocks", Bp, Hz, Wz, Np, pk, ps, pp) if pool_fused else 0
    if nb <= 0:
        lib.call(_k("nasseg_pool_bwd", g), 0, ptr(g), ptr(pool_idx), ptr(g_full), Bp, Hz, Wz, Np,
                 g.shape[2], g.shape[3], pk, ps, pp, s)
        return fl._replace(g=g_full)
    mean, invstd = _bn_parts(last.stats, Np)[:2]
    part = _rows_ws(g, nb, Np)
    lib.call(_k("nasseg_maxpool_bn_bwd", g), ptr(g), ptr(pool_idx), ptr(last.z), ptr(mean), ptr(invstd),
             ptr(g_full), ptr(part), Bp, Hz, Wz, Np, g.shape[2], g.shape[3], ps, pp, s)
    return fl._replace(g=g_full, rows=(part, nb))


# BatchNorm-backward partial rows handed from a consumer's backward to the producer chain's, by the side of
# the gradient tensor: data_ptr -> (weakref to that tensor, rows, number of rows, its version).  An entry is only
# honoured for the very tensor object it was made for (a dead or different object: the chain reduces as usual).
_TAIL_ROWS = {}
FUSE_TAIL_ROWS = os.environ.get("NASSEG_FUSE_TAIL_ROWS", "1") != "0"


def _sweep_tail_rows():
    """drop the rows whose gradient tensor died unconsumed (a backward that stopped short)"""
    for key in [k for k, e in _TAIL_ROWS.items() if e[0]() is None]:
        del _TAIL_ROWS[key]


def _hand_tail_rows(g, rows, nrows):
    """hand the producer chain's backward the rows of its BatchNorm-backward sums that come with gradient ``g``"""
    _sweep_tail_rows()
    _TAIL_ROWS[g.data_ptr()] = (weakref.ref(g), rows, nrows, g._version)


def _take_tail_rows(g):
    """(rows, nrows) handed over with gradient ``g`` - or None, also where g is another object or autograd has since
    accumulated another consumer's gradient into it (its version moved: the chain reduces the sum itself)"""
    ent = _TAIL_ROWS.pop(g.data_ptr(), None)
    if ent is not None and ent[0]() is g and g._version == ent[3]:
        return ent[1], ent[2]
    return None


class Pending(object):
    """A conv chain's raw last conv output whose BatchNorm (+ activation) is still to be applied:
    y = act(scale[c]*z + shift[c]).  A consumer that understands it (cat_reduce) applies the tail as it loads z -
    the normalised map is never written; anything else calls materialize().  Backward contract: the gradient
    that flows back into ``z``'s slot is the one w.r.t. y (the chain's backward is the same either way: it has
    always received dL/dy and redone mask and BatchNorm backward from z)."""

    __slots__ = ("z", "stats", "act", "_mat")

    def __init__(self, z, stats, act):
        self.z, self.stats, self.act = z, stats, int(act)  # stats: mean | invstd | scale | shift, C each
        self._mat = None

    scale = property(lambda self: _scale_shift(self.stats, self.z.shape[1])[0])
    shift = property(lambda self: _scale_shift(self.stats, self.z.shape[1])[1])
    shape = property(lambda self: self.z.shape)
    dtype = property(lambda self: self.z.dtype)
    device = property(lambda self: self.z.device)

    def size(self, *a):
        return self.z.size(*a)

    def dim(self):
        return self.z.dim()

    def materialize(self):
        # (memoised: a node with several consumers that cannot apply the tail themselves is normalised once)
        if self._mat is None:
            self._mat = _ApplyTail.apply(self.z, self.scale, self.shift, self.act)
        return self._mat


class _ApplyTail(torch.autograd.Function):
    """The pass a deferred tail avoided: y = act(scale*z + shift); the gradient goes through unchanged (see
    Pending: z's slot carries dL/dy)."""

    @staticmethod
    def forward(ctx, z, scale, shift, act):
        return _affine_act(_cl(z), scale, shift, None, act)

    @staticmethod
    def backward(ctx, dy):
        return dy, None, None, None


def materialize(x):
    """A plain tensor from a tensor or a Pending."""
    return x.materialize() if isinstance(x, Pending) else x


# Nodes with several consumers (a cell's node read by several ops and sums, a decoder map read by several blocks and
# collect_all: src/nn/micro_decoders.py:95-121,237-251,380-398) go through ONE gradient junction instead of autograd's
# pairwise accumulation (an at::native add launch and three tensor passes per extra consumer) - and a junction over a
# Pending node also does the mask-and-reduce pass of its producer's BatchNorm backward.  NASSEG_JUNCTION=0: as before.
JUNCTION = os.environ.get("NASSEG_JUNCTION", "1") != "0"
_JUNCTION_MAX = 8  # gradients one nasseg_grad_junction launch adds


class _Junction(torch.autograd.Function):
    """Fan a node out to its consumers.  forward(z, stats, act, n_raw, n_fin): n_raw aliases of z for consumers that
    take the node as it is - a plain tensor (stats None), or a conv chain's raw output whose BatchNorm + activation they
    apply on load (the caller wraps them into Pending objects) - and n_fin aliases of the FINISHED map act(scale*z +
    shift), written once, for consumers that need it.  Backward: whatever gradients came back (all of them w.r.t. the
    finished value: Pending's contract) are added by one nasseg_grad_junction launch; over a pending node the sum is
    also multiplied by act' (a contribution that arrived masked stays as it is: the mask is 0 / 1) and comes with the
    producer's BatchNorm-backward sums as rows, handed to the chain's backward by the side of the gradient
    (_TAIL_ROWS) - which then skips its own pass over gradient and z."""

    @staticmethod
    def forward(ctx, z, stats, act, n_raw, n_fin):
        z = _cl(z)
        C = z.shape[1]
        fin = None
        if n_fin:
            fin = z if stats is None else _affine_act(z, *_scale_shift(stats, C), None, act)
        outs = [z.view_as(z) for _ in range(n_raw)] + [fin.view_as(fin) for _ in range(n_fin)]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(z if stats is not None else None, stats)
        ctx.cfg = (int(act), tuple(z.shape), z.dtype, z.device)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        z, stats = ctx.saved_tensors
        act, shape, dtype, device = ctx.cfg
        live = [_cl(g) for g in grads if g is not None]
        if not live:
            return None, None, None, None, None
        if len(live) == 1 and stats is None:
            return live[0], None, None, None, None
        B, C, H, W = shape
        s = current_stream()
        nrows = lib.query("nasseg_cat_src_blocks", B, H, W, C)
        if nrows <= 0:  # (a width the row layout does not serve: C / 4 > 256)
            out = live[0]
            for g in live[1:]:
                out = _axpby(out, g, None, None)
            return out, None, None, None, None
        # more than eight consumers: partial sums first (plain adds), the mask and the rows with the last launch
        while len(live) > _JUNCTION_MAX:
            head, live = live[:_JUNCTION_MAX], live[_JUNCTION_MAX:]
            part_sum = torch.empty_like(head[0])
            lib.call(_k("nasseg_grad_junction", head[0]), *([ptr(g) for g in head] + [len(head), None, None, ACT_NONE,
                     ptr(part_sum), None, B, H, W, C, s]))
            live.insert(0, part_sum)
        # (a pending node whose only gradient came from one consumer: the mask and the rows alone, n = 1)
        out = torch.empty(shape, device=device, dtype=dtype, memory_format=torch.channels_last)
        rows = _rows_ws(out, nrows, C) if (stats is not None and FUSE_TAIL_ROWS) else None
        args = [ptr(g) for g in live] + [None] * (_JUNCTION_MAX - len(live))
        lib.call(_k("nasseg_grad_junction", out), *(args + [len(live), ptr(z) if stats is not None else None,
                 ptr(stats), act, ptr(out), ptr(rows), B, H, W, C, s]))
        if rows is not None:
            _hand_tail_rows(out, rows, nrows)
        return out, None, None, None, None


def fan_out(x, n_raw, n_fin=0):
    """Handles of a node for its consumers: ``n_raw`` that take it as it is (x itself, or - x a Pending - Pending
    objects whose tail the consumer applies on load) followed by ``n_fin`` finished maps (plain tensors).  With one
    consumer in all, a width the junction kernel does not serve, no gradient to route, or NASSEG_JUNCTION=0 the
    handles are x itself / its memoised materialisation: autograd accumulates as it always did."""
    n = n_raw + n_fin
    pending = isinstance(x, Pending)
    z = x.z if pending else x
    if (n < 2 or not JUNCTION or z.dim() != 4 or z.shape[1] % 4 != 0 or not torch.is_grad_enabled()
            or not z.requires_grad):
        return [x] * n_raw + [materialize(x)] * n_fin if n_fin else [x] * n_raw
    if pending:
        outs = _Junction.apply(x.z, x.stats, x.act, n_raw, n_fin)
        return [Pending(t, x.stats, x.act) for t in outs[:n_raw]] + list(outs[n_raw:])
    return list(_Junction.apply(x, None, ACT_NONE, n, 0))


def conv_chain(x, ops, in_act0=ACT_NONE, residual=None, pool=None, defer_tail=False):
    """ops: list of (weight, stride, padding, dilation, depthwise, bn, act) where ``bn`` is None
    or (gamma, beta, running_mean, running_var, num_batches_tracked, training, momentum, eps).
    pool = (3, stride, 1): 3x3 max pooling of the chain's output (which must end in a BatchNorm without
    activation and without residual - the reference's Pool op), fused behind it.
    defer_tail: return a Pending (raw conv output + the last BatchNorm's scale/shift + activation) instead of
    the normalised output when the chain ends in a BatchNorm that is not folded (no residual, no pooling)."""
    cfg_ops, tensors = [], []
    for weight, stride, padding, dilation, depthwise, bn, act in ops:
        gamma, beta, rm, rv, nbt, training, momentum, eps = bn if bn is not None else (None,) * 5 + (False, 0.0, 0.0)
        cfg_ops.append(_ChainOp("dw" if depthwise else "dense", int(stride), int(padding), int(dilation),
                                bn is not None, int(act) if bn is not None else ACT_NONE, bool(training),
                                float(momentum), float(eps)))
        tensors.extend([weight, gamma, beta, rm, rv, nbt if training else None])
    in_st = in_pact = None
    if isinstance(x, Pending):
        if in_act0 != ACT_NONE or not cfg_ops:
            x = x.materialize()  # (an activation on top of a pending one: not fused)
        else:
            x, in_st, in_pact = x.z, x.stats, x.act
    defer = bool(defer_tail and residual is None and pool is None and cfg_ops and cfg_ops[-1].has_bn)
    cfg = _ChainCfg(int(in_act0), tuple(cfg_ops), torch.is_grad_enabled(),
                    (int(pool[0]), int(pool[1]), int(pool[2])) if pool is not None else None, defer, in_pact)
    out = _ConvChain.apply(cfg, x, residual, *(tensors + [in_st]))
    if not defer:
        return out
    y, stats = out
    return y if stats is None else Pending(y, stats, cfg_ops[-1].act)


def conv_bn_act(x, weight, gamma, beta, running_mean, running_var, num_batches_tracked, training,
                momentum=0.1, eps=1e-5, act=ACT_NONE, residual=None, stride=1, padding=0, dilation=1):
    """act(BN(conv(x))) (+ residual): a conv chain of one link (statistics in the conv epilogue;
    in inference without grad the BatchNorm is folded into the conv's epilogue - one kernel)."""
    bn = (gamma, beta, running_mean, running_var, num_batches_tracked, bool(training), momentum, eps)
    return conv_chain(x, [(weight, stride, padding, dilation, False, bn, int(act))], ACT_NONE, residual)


# ---------------------------------------------------------------------------
# BatchNorm (+ activation, + residual)
# ---------------------------------------------------------------------------
class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, nbt, training, momentum, eps, act,
                residual):
        x = _cl(x)
        B, C, H, W = x.shape
        stats, _, _, scale, shift = _bn_head(x, C, B * H * W, x.shape, (gamma, beta, running_mean, running_var, nbt),
                                             training, momentum, eps, x)
        res = _cl(residual) if residual is not None else None
        y = _affine_act(x, scale, shift, res, act)
        ctx.save_for_backward(x, stats)
        ctx.cfg = (bool(training), act, residual is not None, gamma is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stats = ctx.saved_tensors
        training, act, has_res, affine = ctx.cfg
        dy = _cl(dy)
        B, C, H, W = x.shape
        M = B * H * W
        mean, invstd, scale, shift = _bn_parts(stats, C)
        s = current_stream()
        sums = _vec(x, 2 * C)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        rows = _bn_bwd_reduce(dy, x, scale, shift, mean, invstd, act, sums, M, C, dx is not None and C % 4 == 0)
        if dx is not None:
            _bn_bwd_apply(dy, x, scale, shift, mean, invstd, sums, M, C, training, act, dx, rows)
        dgamma = sums[C:2 * C] if (affine and ctx.needs_input_grad[1]) else None
        dbeta = sums[0:C] if (affine and ctx.needs_input_grad[2]) else None
        dres = dy if (has_res and ctx.needs_input_grad[10]) else None
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, dres


def batch_norm_act(x, gamma, beta, running_mean, running_var, num_batches_tracked, training,
                   momentum=0.1, eps=1e-5, act=ACT_NONE, residual=None):
    """y = act(BN(x)) (+ residual).  Training mode updates the running buffers in place."""
    return _BatchNormAct.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked,
                               bool(training), momentum, eps, int(act), residual)


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------
class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode, k, stride, pad):
        x = _cl(x)
        B, C, H, W = x.shape
        Ho, Wo = conv_out_size(H, k, stride, pad, 1), conv_out_size(W, k, stride, pad, 1)
        y = _new(x, B, C, Ho, Wo)
        idx = None
        if mode == 0:
            idx = torch.empty((B, Ho, Wo, C), device=x.device, dtype=torch.uint8)
        lib.call(_k("nasseg_pool_fwd", x), mode, ptr(x), ptr(y), ptr(idx), B, H, W, C, Ho, Wo, k, stride,
                 pad, current_stream())
        ctx.cfg = (mode, k, stride, pad, (B, C, H, W))
        ctx.idx = idx
        return y

    @staticmethod
    def backward(ctx, dy):
        mode, k, stride, pad, (B, C, H, W) = ctx.cfg
        dy = _cl(dy)
        dx = _new(dy, B, C, H, W)
        lib.call(_k("nasseg_pool_bwd", dy), mode, ptr(dy), ptr(ctx.idx), ptr(dx), B, H, W, C, dy.shape[2],
                 dy.shape[3], k, stride, pad, current_stream())
        return dx, None, None, None, None


def max_pool2d(x, kernel_size=3, stride=1, padding=1):
    return _Pool.apply(x, 0, int(kernel_size), int(stride), int(padding))


def avg_pool2d(x, kernel_size=3, stride=1, padding=1):
    """count_include_pad=False semantics."""
    return _Pool.apply(x, 1, int(kernel_size), int(stride), int(padding))


# ---------------------------------------------------------------------------
# bilinear resize, concat
# ---------------------------------------------------------------------------
class _Bilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo):
        x = _cl(x)
        B, C, H, W = x.shape
        y = _new(x, B, C, Ho, Wo)
        lib.call(_k("nasseg_bilinear_fwd", x), ptr(x), ptr(y), C, 0, B, H, W, C, Ho, Wo, ACT_NONE,
                 current_stream())
        ctx.shape = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        dy = _cl(dy)
        dx = _new(dy, B, C, H, W)
        nws = lib.query("nasseg_bilinear_bwd_workspace", B, H, W, C, dy.shape[2], dy.shape[3])
        lib.call(_k("nasseg_bilinear_bwd", dy), ptr(dy), C, 0, ptr(dx), B, H, W, C, dy.shape[2],
                 dy.shape[3], ptr(_ws(dy, nws)) if nws else None, current_stream())
        return dx, None, None


def bilinear_resize(x, size, align_corners=False):
    """nn.Upsample(size, mode='bilinear') / F.interpolate(..., align_corners=False); align_corners=True
    (the distillation teacher's decoder, src/kd/rf_lw/model_lw_v2.py:258) is forward-only."""
    Ho, Wo = int(size[0]), int(size[1])
    if tuple(x.shape[2:]) == (Ho, Wo):
        return x
    if align_corners:
        if x.requires_grad and torch.is_grad_enabled():
            raise NassegError("bilinear_resize(align_corners=True) has no backward (inference-only)")
        x = _cl(x)
        B, C, H, W = x.shape
        if C % 4 != 0:
            raise NassegError("bilinear_resize(align_corners=True): C % 4 != 0")
        y = _new(x, B, C, Ho, Wo)
        lib.call(_k("nasseg_bilinear_ac_fwd", x), ptr(x), ptr(y), B, H, W, C, Ho, Wo, current_stream())
        return y
    return _Bilinear.apply(x, Ho, Wo)


class _ConcatResize(torch.autograd.Function):
    """cat(dim=1) of tensors, each bilinearly resized to (Ho, Wo) when needed,
    written straight into the output slab, with an optional fused ReLU."""

    @staticmethod
    def forward(ctx, Ho, Wo, act, *xs):
        xs = [_cl(x) for x in xs]
        B = xs[0].shape[0]
        Ct = sum(x.shape[1] for x in xs)
        y = _new(xs[0], B, Ct, Ho, Wo)
        s = current_stream()
        off = 0
        shapes = []
        for x in xs:
            _, C, H, W = x.shape
            if x.shape[0] != B:
                raise NassegError("concat: batch sizes differ")
            if (H, W) == (Ho, Wo):
                lib.call(_k("nasseg_chan_copy", x), ptr(x), C, 0, ptr(y), Ct, off, None, 0, 0, B * Ho * Wo,
                         C, act, ACT_NONE, s)
            else:
                lib.call(_k("nasseg_bilinear_fwd", x), ptr(x), ptr(y), Ct, off, B, H, W, C, Ho, Wo, act, s)
            shapes.append((C, H, W))
            off += C
        ctx.shapes = shapes
        ctx.act = act
        if act != ACT_NONE:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _cl(dy)
        B, Ct, Ho, Wo = dy.shape
        s = current_stream()
        if ctx.act != ACT_NONE:
            (y,) = ctx.saved_tensors
            dy = _act_bwd(dy, y, ctx.act)
        grads = []
        off = 0
        for i, (C, H, W) in enumerate(ctx.shapes):
            if not ctx.needs_input_grad[3 + i]:
                grads.append(None)
                off += C
                continue
            dx = _new(dy, B, C, H, W)
            if (H, W) == (Ho, Wo):
                lib.call(_k("nasseg_chan_copy", dy), ptr(dy), Ct, off, ptr(dx), C, 0, None, 0, 0,
                         B * Ho * Wo, C, ACT_NONE, ACT_NONE, s)
            else:
                nws = lib.query("nasseg_bilinear_bwd_workspace", B, H, W, C, Ho, Wo)
                lib.call(_k("nasseg_bilinear_bwd", dy), ptr(dy), Ct, off, ptr(dx), B, H, W, C, Ho, Wo,
                         ptr(_ws(dy, nws)) if nws else None, s)
            grads.append(dx)
            off += C
        return (None, None, None) + tuple(grads)


def concat_resize(tensors, size, relu=False):
    return _ConcatResize.apply(int(size[0]), int(size[1]), ACT_RELU if relu else ACT_NONE, *tensors)


def _bn_relu_pw_forward(x, scale, shift, wp, N, res=None):
    """conv1x1(relu(scale * x + shift)) (+ res) with the BatchNorm + ReLU applied as the conv loads x (the normalised
    map is never written); wp: the (N, C, 1, 1) weight packed for the forward (_pack_dense mode 0)"""
    B, C, H, W = x.shape
    out = _new(x, B, N, H, W)
    lib.call(_k("nasseg_conv_fwd", x), ptr(x), C, ptr(wp), ptr(out), N, ptr(scale), ptr(shift), ACT_RELU, None, None,
             ACT_NONE, ptr(res), N if res is not None else 0, B, H, W, C, H, W, N, 1, 1, 1, 0, 1, 0, None,
             current_stream())
    return out


def _bn_relu_pw_backward(dout, x, parts, wb):
    """Backward of _bn_relu_pw_forward up to the BatchNorm: the backward-data kernel (wb: the weight packed mode 1)
    leaves g = relu'(bn(x)) * backward_data(dout) with the rows of the BatchNorm-backward sums {sum g, sum g * xhat} -
    no reduction pass over gradient and x.  Returns (g, sums); parts = (mean, invstd, scale, shift)."""
    mean, invstd, scale, shift = parts
    B, C, H, W = x.shape
    N = dout.shape[1]
    s = current_stream()
    nb = lib.query("nasseg_conv_fwd_stats_blocks", B, H, W, C, N, 2)
    g = _new(x, B, C, H, W)
    part = _rows_ws(x, nb, C)
    lib.call(_k("nasseg_conv_bwd_data_bn", dout), ptr(dout), N, ptr(wb), ptr(g), C, ptr(x), C, ptr(scale), ptr(shift),
             ptr(mean), ptr(invstd), ACT_RELU, B, H, W, N, H, W, C, 1, 1, 1, 0, 1, ptr(part), s)
    sums = _vec(x, 2 * C)
    lib.call("nasseg_rows_sum", ptr(part), nb, 2 * C, ptr(sums), s)
    return g, sums


def _bn_relu_pw_dx(g, x, parts, sums, training):
    """dx of the plain BatchNorm backward from what _bn_relu_pw_backward left (g arrived masked: ACT_NONE, the rule of
    _ChainBackward.bn_head)"""
    mean, invstd, scale, shift = parts
    B, C, H, W = x.shape
    return _bn_bwd_apply(g, x, scale, shift, mean, invstd, sums, B * H * W, C, training, ACT_NONE, torch.empty_like(x))


class _CatBNReluConv(torch.autograd.Function):
    """ConcatReduce's tail, cat(x, y) -> BatchNorm(2C) -> ReLU -> 1x1 conv (2C -> N)
    (src/nn/layer_factory.py:369-382), WITHOUT the concatenation: BatchNorm is per channel and
    the 1x1 conv is linear in its input channels, so

        out = W[:, :C] . relu(bn_lo(x)) + W[:, C:] . relu(bn_hi(y))

    Two pointwise convs (_bn_relu_pw_*), each over its half of the BatchNorm (the second adds the
    first's output in its epilogue); neither the 2C-channel slab nor its normalised copy is ever
    written, and the backward needs no slicing.  Used for large maps (a few more, smaller
    launches than the slab path)."""

    @staticmethod
    def forward(ctx, x, y, gamma, beta, rm, rv, nbt, weight, training, momentum, eps, grad_mode=True):
        x, y = _cl(x), _cl(y)
        B, C, H, W = x.shape
        N = weight.shape[0]
        w = weight.contiguous()
        if tuple(y.shape) != (B, C, H, W) or tuple(w.shape) != (N, 2 * C, 1, 1):
            raise NassegError("cat_bn_relu_conv: shapes {} {} {}".format(
                tuple(x.shape), tuple(y.shape), tuple(w.shape)))
        M = B * H * W
        needs_grad = grad_mode and any(ctx.needs_input_grad)  # (grad_mode: the caller's, see _ConvChain)
        stats, parts = _bn_alloc(x, 2 * C, training, M, (B, 2 * C, H, W))  # [mean | invstd | scale | shift] x [2C]
        if training:
            # each half's statistics into its columns of the 2C vector; num_batches_tracked moves once, with the first
            for lo, t, n in ((0, x, nbt), (C, y, None)):
                cols = [None if v is None else v[lo:lo + C] for v in (gamma, beta, rm, rv)] + [n]
                _bn_fill([v[lo:lo + C] for v in parts], C, M, cols, True, momentum, eps, t)
        else:
            _bn_fill(parts, 2 * C, M, (gamma, beta, rm, rv, nbt), False, momentum, eps)
        scale, shift = parts[2:]
        items = [(w, 0, 0, C), (w, 0, C, C)]
        if needs_grad:
            items += [(w, 1, 0, C), (w, 1, C, C)]
        packed = _pack_many(x, items)
        y1 = _bn_relu_pw_forward(x, scale[0:C], shift[0:C], packed[0], N)
        out = _bn_relu_pw_forward(y, scale[C:], shift[C:], packed[1], N, y1)
        if needs_grad:
            ctx.save_for_backward(x, y, stats, packed[2], packed[3])
            ctx.cfg = (bool(training), N)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y, stats, wb_lo, wb_hi = ctx.saved_tensors
        training, N = ctx.cfg
        dout = _cl(dout)
        B, C, H, W = x.shape
        s = current_stream()
        parts = _bn_parts(stats, 2 * C)
        need_w = ctx.needs_input_grad[7]
        need_bn = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        dbn = _vec(x, 4 * C) if need_bn else None  # [dbeta(2C) | dgamma(2C)]
        dw = torch.empty((N, 2 * C, 1, 1), device=x.device, dtype=torch.float32) if need_w else None
        grads_in = [None, None]
        for h, (t, wb) in enumerate(((x, wb_lo), (y, wb_hi))):
            lo = h * C
            half = [v[lo:lo + C] for v in parts]
            if ctx.needs_input_grad[h] or need_bn:
                g, sums = _bn_relu_pw_backward(dout, t, half, wb)
                if need_bn:  # sums = [sum g | sum g*xhat] -> rows (dbeta, dgamma) of dbn at columns lo..lo + C
                    lib.call(_k("nasseg_chan_copy", sums), ptr(sums), C, 0, ptr(dbn), 2 * C, lo, None, 0, 0, 2, C,
                             ACT_NONE, ACT_NONE, s)
                if ctx.needs_input_grad[h]:
                    grads_in[h] = _bn_relu_pw_dx(g, t, half, sums, training)
            if need_w:
                # (launched here and not through _dense_wgrad: a half's gradient is gathered into dw's columns by the
                #  copy below, which a finalisation deferred to the end of backward - deferred_wgrad - would come after)
                dwh = _vec(x, N * C)
                ws = _ws(x, lib.query("nasseg_conv_wgrad_workspace", B, H, W, N, C, 1, 1))
                lib.call(_k("nasseg_conv_wgrad", t), ptr(t), C, ptr(dout), N, ptr(dwh), ptr(ws), ptr(half[2]),
                         ptr(half[3]), ACT_RELU, B, H, W, C, H, W, N, 1, 1, 1, 0, 1, s)
                lib.call(_k("nasseg_chan_copy", dwh), ptr(dwh), C, 0, ptr(dw), 2 * C, lo, None, 0, 0, N, C, ACT_NONE,
                         ACT_NONE, s)
        dgamma = dbn[2 * C:4 * C] if ctx.needs_input_grad[2] else None
        dbeta = dbn[0:2 * C] if ctx.needs_input_grad[3] else None
        return (grads_in[0], grads_in[1], dgamma, dbeta, None, None, None, dw, None, None, None, None)


def cat_bn_relu_conv(x, y, gamma, beta, running_mean, running_var, num_batches_tracked, weight,
                     training, momentum=0.1, eps=1e-5):
    """conv1x1(relu(batch_norm(cat([x, y], 1)))) without materialising the concatenation."""
    return _CatBNReluConv.apply(x, y, gamma, beta, running_mean, running_var, num_batches_tracked,
                                weight, bool(training), float(momentum), float(eps), torch.is_grad_enabled())


class _BNReluConv(torch.autograd.Function):
    """BatchNorm -> ReLU -> 1x1 conv over ONE tensor (ConcatReduce's tail on its concat slab,
    src/nn/layer_factory.py:369-382, below the size where the slab is avoided altogether): _bn_relu_pw_* over
    the tensor's own statistics.  The single-input form of _CatBNReluConv."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, weight, training, momentum, eps, grad_mode):
        x = _cl(x)
        B, C, H, W = x.shape
        N = weight.shape[0]
        w = weight.contiguous()
        if tuple(w.shape) != (N, C, 1, 1):
            raise NassegError("bn_relu_conv: shapes {} {}".format(tuple(x.shape), tuple(w.shape)))
        needs_grad = grad_mode and any(ctx.needs_input_grad)
        stats, _, _, scale, shift = _bn_head(x, C, B * H * W, x.shape, (gamma, beta, rm, rv, nbt), training, momentum,
                                             eps, x)
        packed = _pack_many(x, [(w, 0), (w, 1)] if needs_grad else [(w, 0)])
        out = _bn_relu_pw_forward(x, scale, shift, packed[0], N)
        if needs_grad:
            ctx.save_for_backward(x, stats, packed[1], w)
            ctx.cfg = (bool(training), N)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, stats, wb, w = ctx.saved_tensors
        training, N = ctx.cfg
        dout = _cl(dout)
        B, C, H, W = x.shape
        parts = _bn_parts(stats, C)
        dx = dgamma = dbeta = dw = None
        if any(ctx.needs_input_grad[0:3]):
            g, sums = _bn_relu_pw_backward(dout, x, parts, wb)
            dgamma = sums[C:2 * C] if ctx.needs_input_grad[1] else None
            dbeta = sums[0:C] if ctx.needs_input_grad[2] else None
            if ctx.needs_input_grad[0]:
                dx = _bn_relu_pw_dx(g, x, parts, sums, training)
        if ctx.needs_input_grad[6]:
            dw = _dense_wgrad(x, dout, w, parts[2], parts[3], ACT_RELU, (B, H, W, C, H, W, N, 1, 1, 1, 0, 1))
        return dx, dgamma, dbeta, None, None, None, dw, None, None, None, None


class _CatReduce(torch.autograd.Function):
    """ConcatReduce whole (src/nn/layer_factory.py:369-382 with Adapt's resize, :338-350) as ONE node:
    cat(x, y) -> BatchNorm(2C) -> ReLU -> 1x1 conv.  Each input is written into its half of the slab by one
    launch (nasseg_cat_src_fwd) that resizes it when its size differs, applies the producer's pending
    BatchNorm + activation on load (Pending: the producers' normalised outputs are never written) and emits
    the slab's BatchNorm statistics as partial rows - no pass over the slab for them; the conv is
    _bn_relu_pw_forward over the slab.  Backward: _bn_relu_pw_backward leaves the masked gradient + the slab
    BatchNorm's sums; nasseg_cat_src_bwd then applies that BatchNorm's backward per input
    slice (no full-width slab gradient), and for a pending input of the slab's size also masks with its
    activation's derivative and emits the producer's BatchNorm-backward sums (_TAIL_ROWS).  The gradient
    returned for a Pending input is the one w.r.t. its activated output (the producer chain's backward takes
    it from there).

    cfg = (Ho, Wo, act_x, act_y, training, momentum, eps, grad_mode); xst / yst: the producers' statistics
    vectors (mean | invstd | scale | shift) or None."""

    @staticmethod
    def forward(ctx, cfg, x, y, xst, yst, gamma, beta, rm, rv, nbt, weight):
        Ho, Wo, act_x, act_y, training, momentum, eps, grad_mode = cfg
        x, y = _cl(x), _cl(y)
        B, C = x.shape[0], x.shape[1]
        Ct = 2 * C
        N = weight.shape[0]
        w = weight.contiguous()
        if y.shape[0] != B or y.shape[1] != C or tuple(w.shape) != (N, Ct, 1, 1):
            raise NassegError("cat_reduce: shapes {} {} {}".format(tuple(x.shape), tuple(y.shape), tuple(w.shape)))
        M = B * Ho * Wo
        s = current_stream()
        needs_grad = grad_mode and any(ctx.needs_input_grad)
        stats, parts = _bn_alloc(x, Ct, training, M, (B, Ct, Ho, Wo))
        slab = _new(x, B, Ct, Ho, Wo)
        nblk = lib.query("nasseg_cat_src_blocks", B, Ho, Wo, C)
        part = _rows_ws(x, nblk, Ct) if training else None
        for off, (t, st, act) in enumerate(((x, xst, act_x), (y, yst, act_y))):
            sc, sh = _scale_shift(st, C)
            lib.call(_k("nasseg_cat_src_fwd", t), ptr(t), ptr(sc), ptr(sh), act if st is not None else ACT_NONE,
                     ptr(slab), Ct, off * C, ptr(part), B, t.shape[2], t.shape[3], C, Ho, Wo, s)
        _bn_fill(parts, Ct, M, (gamma, beta, rm, rv, nbt), training, momentum, eps, rows=(part, nblk))
        packed = _pack_many(x, [(w, 0), (w, 1)] if needs_grad else [(w, 0)])
        out = _bn_relu_pw_forward(slab, parts[2], parts[3], packed[0], N)
        if needs_grad:
            # (x / y: the producers' raw outputs - they hold them for their own backward anyway)
            ctx.save_for_backward(slab, stats, packed[1], w, x if xst is not None else None,
                                  y if yst is not None else None, xst, yst)
            ctx.cfg = (bool(training), N, tuple(x.shape), tuple(y.shape), act_x, act_y)
        return out

    @staticmethod
    def backward(ctx, dout):
        _sweep_tail_rows()
        slab, stats, wb, w, zx, zy, xst, yst = ctx.saved_tensors
        training, N, x_shape, y_shape, act_x, act_y = ctx.cfg
        dout = _cl(dout)
        B, Ct, Ho, Wo = slab.shape
        C = Ct // 2
        s = current_stream()
        mean, invstd, scale, shift = parts = _bn_parts(stats, Ct)
        need_in = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need_bn = ctx.needs_input_grad[5] or ctx.needs_input_grad[6]
        dx = dy = dgamma = dbeta = dw = None
        if need_in or need_bn:
            g, sums = _bn_relu_pw_backward(dout, slab, parts, wb)
            dgamma = sums[Ct:2 * Ct] if ctx.needs_input_grad[5] else None
            dbeta = sums[0:Ct] if ctx.needs_input_grad[6] else None
            if need_in:
                nrows = lib.query("nasseg_cat_src_blocks", B, Ho, Wo, C)
                grads = []
                for off, (need, shp, z, st, act) in enumerate(((ctx.needs_input_grad[1], x_shape, zx, xst, act_x),
                                                               (ctx.needs_input_grad[2], y_shape, zy, yst, act_y))):
                    if not need:
                        grads.append(None)
                        continue
                    _, _, H, W = shp
                    same = (H, W) == (Ho, Wo)
                    # the producer's mask and BatchNorm-backward sums ride along: directly when its output has the
                    # slab's size; behind a resize the sums are formed at the slab's size against the interpolated
                    # mask and nasseg_bilinear_bwd_act masks the gradient it transposes
                    # (a producer SMALLER than the slab keeps its own reduction pass: over its few pixels that is
                    #  cheaper than four taps of z per slab pixel - 3 launches of the headline step, +15 us each)
                    rows = (_rows_ws(slab, nrows, C)
                            if (st is not None and FUSE_TAIL_ROWS and H * W >= Ho * Wo) else None)
                    d = _new(slab, B, C, Ho, Wo)
                    lib.call(_k("nasseg_cat_src_bwd", g), ptr(g), ptr(slab), Ct, off * C, ptr(scale), ptr(mean),
                             ptr(invstd), ptr(sums), int(training), ptr(z) if rows is not None else None,
                             ptr(st) if rows is not None else None, act, ptr(d), ptr(rows), B, Ho, Wo, C,
                             H if rows is not None else Ho, W if rows is not None else Wo, s)
                    if not same:
                        full = _new(slab, B, C, H, W)
                        nws = lib.query("nasseg_bilinear_bwd_workspace", B, H, W, C, Ho, Wo)
                        ws = ptr(_ws(d, nws)) if nws else None
                        if rows is not None:
                            sc, sh = _scale_shift(st, C)
                            lib.call(_k("nasseg_bilinear_bwd_act", d), ptr(d), C, 0, ptr(z), ptr(sc), ptr(sh), act,
                                     ptr(full), B, H, W, C, Ho, Wo, ws, s)
                        else:
                            lib.call(_k("nasseg_bilinear_bwd", d), ptr(d), C, 0, ptr(full), B, H, W, C, Ho, Wo, ws, s)
                        d = full
                    if rows is not None:
                        _hand_tail_rows(d, rows, nrows)
                    grads.append(d)
                dx, dy = grads
        if ctx.needs_input_grad[10]:
            dw = _dense_wgrad(slab, dout, w, scale, shift, ACT_RELU, (B, Ho, Wo, Ct, Ho, Wo, N, 1, 1, 1, 0, 1))
        return None, dx, dy, None, None, dgamma, dbeta, None, None, None, dw


def cat_reduce_ok(x, y, weight):
    """Shapes _CatReduce serves: both inputs of the same width C (a multiple of 4; what Adapt leaves), a 1x1
    conv over 2C channels with N % 4 == 0 outputs."""
    C = x.shape[1]
    return (FUSE_CAT_REDUCE and C == y.shape[1] and C % 4 == 0 and C // 4 <= 256 and weight.shape[0] % 4 == 0
            and x.shape[0] == y.shape[0])


def cat_reduce(x, y, size, gamma, beta, running_mean, running_var, num_batches_tracked, weight, training,
               momentum=0.1, eps=1e-5):
    """conv1x1(relu(batch_norm(cat(resize(x), resize(y))))) with ``size`` the common (H, W); x / y: tensors or
    Pending outputs of conv chains (their BatchNorm + activation are then applied as the slab is written)."""
    parts = []
    for t in (x, y):
        parts.append((t.z, t.stats, t.act) if isinstance(t, Pending) else (t, None, ACT_NONE))
    cfg = (int(size[0]), int(size[1]), parts[0][2], parts[1][2], bool(training), float(momentum), float(eps),
           torch.is_grad_enabled())
    return _CatReduce.apply(cfg, parts[0][0], parts[1][0], parts[0][1], parts[1][1], gamma, beta, running_mean,
                            running_var, num_batches_tracked, weight)


def bn_relu_conv(x, gamma, beta, running_mean, running_var, num_batches_tracked, weight, training,
                 momentum=0.1, eps=1e-5):
    """conv1x1(relu(batch_norm(x))) without materialising the normalised tensor."""
    return _BNReluConv.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, weight,
                             bool(training), float(momentum), float(eps), torch.is_grad_enabled())


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------
class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _cl(a), _cl(b)
        if a.shape != b.shape:
            raise NassegError("add: shapes {} and {} differ".format(tuple(a.shape), tuple(b.shape)))
        return _axpby(a, b, None, None)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def _add_act2(who, za, sta, act_a, a, zb, stb, act_b, b):
    """a[c] * act_a(bn_a(za)) + b[c] * act_b(bn_b(zb)) in one launch: the BatchNorms of the statistics vectors sta /
    stb (None: a finished map) are applied as the raw conv outputs are loaded; a / b None: unit coefficients"""
    if za.shape != zb.shape:
        raise NassegError("{}: shapes {} and {} differ".format(who, tuple(za.shape), tuple(zb.shape)))
    C = za.shape[1]
    y = torch.empty_like(za)
    (sa, ha), (sb, hb) = _scale_shift(sta, C), _scale_shift(stb, C)
    lib.call(_k("nasseg_add_act2", za), ptr(za), ptr(sa), ptr(ha), act_a, ptr(a), ptr(zb), ptr(sb), ptr(hb), act_b,
             ptr(b), ptr(y), za.numel(), C, current_stream())
    return y


class _AddPending(torch.autograd.Function):
    """a + b where one or both are conv-chain outputs with a pending BatchNorm + activation (Pending): the tails
    are applied as the raw conv outputs are loaded (nasseg_add_act2) - one launch and three tensor passes instead
    of up to three launches and seven passes.  Backward: the gradient w.r.t. a sum's operands is the incoming one -
    and a Pending's slot carries the gradient w.r.t. its NORMALISED value (see Pending), so nothing is computed.
    (Masking the operands' gradients here with their chains' BatchNorm-backward rows by the side - nasseg_psum_bwd
    with unit coefficients - was tried in round 5: on the small maps this runs on it leaves 88 - 336 rows per
    operand, too many for the chains' apply kernels to add up themselves, and the launch count went UP by 4.)"""

    @staticmethod
    def forward(ctx, za, zb, sta, stb, act_a, act_b):
        return _add_act2("add", _cl(za), sta, act_a, None, _cl(zb), stb, act_b, None)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy, None, None, None, None


FUSE_PENDING_ADD = os.environ.get("NASSEG_PENDING_ADD", "1") != "0"


def add(a, b):
    """a + b; operands may be Pending (applied on load) where their width allows the vector kernel"""
    pa, pb = isinstance(a, Pending), isinstance(b, Pending)
    if (pa or pb) and FUSE_PENDING_ADD and a.shape[1] % 4 == 0:
        return _AddPending.apply(a.z if pa else a, b.z if pb else b, a.stats if pa else None, b.stats if pb else None,
                                 a.act if pa else ACT_NONE, b.act if pb else ACT_NONE)
    return _Add.apply(materialize(a), materialize(b))


class _ReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        y = _axpby(x, None, None, None, ACT_RELU)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _act_bwd(_cl(dy), y, ACT_RELU)


def relu(x):
    return _ReLU.apply(x)


class _ParamSum(torch.autograd.Function):
    """a[c]*x + b[c]*y  (ParamSum, src/nn/layer_factory.py:353-366)."""

    @staticmethod
    def forward(ctx, x, y, a, b):
        x, y = _cl(x), _cl(y)
        if x.shape != y.shape:
            raise NassegError("psum: shapes {} and {} differ".format(tuple(x.shape), tuple(y.shape)))
        a, b = a.contiguous(), b.contiguous()
        out = _axpby(x, y, a, b)
        ctx.save_for_backward(x, y, a, b)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, y, a, b = ctx.saved_tensors
        dy = _cl(dy)
        B, C, H, W = x.shape
        dx = _axpby(dy, None, a, None) if ctx.needs_input_grad[0] else None
        dyy = _axpby(dy, None, b, None) if ctx.needs_input_grad[1] else None
        da = db = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            sums = _colred(RED_DOT2, dy, C, x, C, y, C, 1, B * H * W, C)
            da, db = sums[0:C], sums[C:2 * C]
        return dx, dyy, da, db


class _ParamSumPending(torch.autograd.Function):
    """a[c]*x + b[c]*y where x and / or y are conv-chain outputs whose last BatchNorm + activation is pending
    (Pending): forward applies the tails as it loads the raw conv outputs (nasseg_add_act2); backward is ONE kernel
    over the gradient (nasseg_psum_bwd) that leaves, per operand, the masked gradient its chain takes together
    with that chain's BatchNorm-backward sums (handed over by the side of the gradient, _TAIL_ROWS), and the rows of
    the coefficient gradients - instead of two scaling passes, a two-dot reduction and two mask-and-reduce passes."""

    @staticmethod
    def forward(ctx, za, zb, sta, stb, a, b, act_a, act_b):
        za, zb, a, b = _cl(za), _cl(zb), a.contiguous(), b.contiguous()
        y = _add_act2("psum", za, sta, act_a, a, zb, stb, act_b, b)
        ctx.save_for_backward(za, zb, sta, stb, a, b)
        ctx.acts = (act_a, act_b)
        return y

    @staticmethod
    def backward(ctx, dy):
        _sweep_tail_rows()
        za, zb, sta, stb, a, b = ctx.saved_tensors
        act_a, act_b = ctx.acts
        dy = _cl(dy)
        B, C, H, W = za.shape
        s = current_stream()
        nrows = lib.query("nasseg_cat_src_blocks", B, H, W, C)
        ga = torch.empty_like(za) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(zb) if ctx.needs_input_grad[1] else None
        rows_a = _rows_ws(za, nrows, C) if (sta is not None and ga is not None and FUSE_TAIL_ROWS) else None
        rows_b = _rows_ws(zb, nrows, C) if (stb is not None and gb is not None and FUSE_TAIL_ROWS) else None
        cpart = _rows_ws(za, nrows, C)
        if (sta is not None and rows_a is None and ga is not None) or (stb is not None and rows_b is None and gb is not None):
            raise NassegError("psum: pending operands need NASSEG_FUSE_TAIL_ROWS")
        lib.call(_k("nasseg_psum_bwd", dy), ptr(dy), ptr(za), ptr(sta), act_a, ptr(a), ptr(ga), ptr(rows_a), ptr(zb),
                 ptr(stb), act_b, ptr(b), ptr(gb), ptr(rows_b), ptr(cpart), B, H, W, C, s)
        da = db = None
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            sums = _vec(za, 2 * C)
            lib.call("nasseg_rows_sum", ptr(cpart), nrows, 2 * C, ptr(sums), s)
            da, db = sums[0:C], sums[C:2 * C]
        for g, rows in ((ga, rows_a), (gb, rows_b)):
            if rows is not None:
                _hand_tail_rows(g, rows, nrows)
        return ga, gb, None, None, da, db, None, None


FUSE_PENDING_PSUM = os.environ.get("NASSEG_PENDING_PSUM", "1") != "0"


def param_sum(x, y, a, b):
    """a[c]*x + b[c]*y (ParamSum); x / y may be Pending (same size, C % 4 == 0: applied on load)"""
    px, py = isinstance(x, Pending), isinstance(y, Pending)
    if (px or py) and FUSE_PENDING_PSUM and FUSE_TAIL_ROWS and x.shape[1] % 4 == 0 and torch.is_grad_enabled():
        return _ParamSumPending.apply(x.z if px else x, y.z if py else y, x.stats if px else None,
                                      y.stats if py else None, a, b, x.act if px else ACT_NONE, y.act if py else ACT_NONE)
    return _ParamSum.apply(materialize(x), materialize(y), a, b)


class _ChannelRepeat(torch.autograd.Function):
    """x.repeat(1, rep, 1, 1)  (Skip / Zero, src/nn/layer_factory.py:268-297)."""

    @staticmethod
    def forward(ctx, x, rep):
        x = _cl(x)
        B, C, H, W = x.shape
        y = _new(x, B, C * rep, H, W)
        s = current_stream()
        for r in range(rep):
            lib.call(_k("nasseg_chan_copy", x), ptr(x), C, 0, ptr(y), C * rep, r * C, None, 0, 0, B * H * W,
                     C, ACT_NONE, ACT_NONE, s)
        ctx.cfg = (rep, (B, C, H, W))
        return y

    @staticmethod
    def backward(ctx, dy):
        rep, (B, C, H, W) = ctx.cfg
        dy = _cl(dy)
        dx = _new(dy, B, C, H, W)
        lib.call(_k("nasseg_chan_fold", dy), ptr(dy), ptr(dx), B * H * W, C, rep, current_stream())
        return dx, None


def channel_repeat(x, rep):
    if rep == 1:
        # torch's repeat always copies; values are what matter downstream
        return _ChannelRepeat.apply(x, 1)
    return _ChannelRepeat.apply(x, int(rep))


def zeros(like, B, C, H, W):
    """A zero activation that is not connected to the autograd graph."""
    require_device(like)
    y = _new(like, B, C, H, W)
    lib.call(_k("nasseg_fill", y), ptr(y), y.numel(), 0.0, current_stream())
    return y


class _ZeroOf(torch.autograd.Function):
    """The reference's Zero op multiplies a view of x by 0.0 (src/nn/layer_factory.py:286-297):
    its output is zeros but stays CONNECTED to x, so everything upstream receives a zero
    gradient (not None: weight decay and momentum still act on those parameters, and a cell of
    'none' ops only still back-propagates)."""

    @staticmethod
    def forward(ctx, x, C, H, W):
        ctx.shape = tuple(x.shape)
        return zeros(x, x.shape[0], C, H, W)

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        return zeros(dy, B, C, H, W), None, None, None


def zero_of(x, C, H, W):
    """zeros of shape (B, C, H, W) that depend on x with a zero gradient (Zero op)."""
    return _ZeroOf.apply(_cl(x), int(C), int(H), int(W))


# ---------------------------------------------------------------------------
# global average pooling and its broadcast
# ---------------------------------------------------------------------------
class _GlobalAvgPool(torch.autograd.Function):
    """The pooled (B, C, 1, 1) map is ALWAYS fp32, also when the activations are stored in
    bfloat16: what follows it in the reference's op (layer_factory.py:181-195) is a BatchNorm over
    those B values per channel, which amplifies the small differences between the samples' means
    - 8 bits of mantissa would leave nothing of them.  B*C values: storage cost nil."""

    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        B, C, H, W = x.shape
        out = _colred(RED_SUM, x, C, None, 0, None, 0, B, H * W, C, 1.0 / (H * W))
        ctx.shape = (B, C, H, W)
        ctx.dtype = x.dtype
        return out.view(B, C, 1, 1)  # (the reduction is fp32)

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        dy = _to_dtype(dy.contiguous().view(B, C, 1, 1), ctx.dtype)
        # every pixel receives dy / (H*W): a broadcast with a scale
        scale = _vec(dy, C)
        lib.call("nasseg_fill", ptr(scale), C, 1.0 / (H * W), current_stream())
        dx = _new(dy, B, C, H, W)
        lib.call(_k("nasseg_bilinear_fwd", dy), ptr(dy), ptr(dx), C, 0, B, 1, 1, C, H, W, ACT_NONE,
                 current_stream())
        return _axpby(dx, None, scale, None)


def global_avg_pool(x):
    """x.mean(2, keepdim=True).mean(3, keepdim=True) -> (B, C, 1, 1), fp32 whatever x's storage."""
    return _GlobalAvgPool.apply(x)


class _Broadcast(torch.autograd.Function):
    """Bilinear interpolation from a 1x1 map = broadcast over (H, W); the output is stored as
    ``dtype`` (the activation storage of the network), the gradient w.r.t. v keeps v's dtype."""

    @staticmethod
    def forward(ctx, v, H, W, dtype):
        require_device(v)
        B, C = v.shape[0], v.shape[1]
        ctx.vdtype = v.dtype
        v = _to_dtype(v.contiguous().view(B, C, 1, 1), dtype)
        y = _new(v, B, C, H, W)
        lib.call(_k("nasseg_bilinear_fwd", v), ptr(v), ptr(y), C, 0, B, 1, 1, C, H, W, ACT_NONE,
                 current_stream())
        ctx.shape = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        dy = _cl(dy)
        dv = _colred(RED_SUM, dy, C, None, 0, None, 0, B, H * W, C)  # (fp32 sums)
        return _to_dtype(dv.view(B, C, 1, 1), ctx.vdtype), None, None, None


def broadcast_to(v, size, dtype=None):
    return _Broadcast.apply(v, int(size[0]), int(size[1]), dtype if dtype is not None else v.dtype)


# ---------------------------------------------------------------------------
# loss and reward
# ---------------------------------------------------------------------------
def _label_tensor(target, who=None):
    require_device(target)
    if target.dtype == torch.int64:
        return target.contiguous(), 8
    if target.dtype == torch.uint8:
        return target.contiguous(), 1
    raise NassegError("{}labels must be int64 or uint8 (got {})".format("" if who is None else who + ": ",
                                                                        target.dtype))


def _label_rows(who, logits, target, rows):
    """the checks of a label cache (N, H, W) read in place through ``rows``, as ``_depth_inputs`` makes them for a
    depth cache -> N.  An index that can be read without a synchronisation (a host tensor) is checked against [0, N)
    before it is refused for being on the host; on the device the kernels clamp (a memory-safety net)."""
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous():
        raise NassegError("{}: rows must be a contiguous 1-D int64 tensor".format(who))
    if (not torch.is_tensor(target) or target.dtype not in (torch.uint8, torch.int64) or target.dim() != 3
            or target.numel() == 0):
        raise NassegError("{}: with rows, the target must be a uint8 or int64 cache of shape (N, H, W) (got {} "
                          "{})".format(who, getattr(target, "dtype", None), tuple(getattr(target, "shape", ()))))
    n_rows = int(target.shape[0])
    if not torch.is_tensor(logits) or logits.dim() != 4 or rows.shape[0] != logits.shape[0]:
        raise NassegError("{}: one cache row per image expected ({} rows for logits {})".format(
            who, rows.shape[0], tuple(getattr(logits, "shape", ()))))
    if not rows.is_cuda and rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n_rows):
        raise IndexError("{}: cache row index out of range [0, {})".format(who, n_rows))
    require_device(logits, target, rows)
    if not target.is_contiguous():
        raise NassegError("{}: with rows, the label cache must be contiguous (it is read in place)".format(who))
    return n_rows


def _segm_inputs(who, logits, target, weight, same_size=True, rows=None):
    """(logits, target, esz, weight) as the segmentation losses' kernels read them: NHWC logits (B, C, h, w),
    contiguous labels of ``esz`` bytes and the logits' size (``same_size=False``: (B, H, W) of any size; with
    ``rows`` a cache (N, H, W) as it stands - _label_rows), fp32 class weights (C,) or None.  ``who``: the public
    function the user called, named by every NassegError."""
    if rows is not None:  # (the cache's dtype and shape, the table's length: before anything else)
        _label_rows(who, logits, target, rows)
    logits = _cl(logits)
    B, C, H, W = logits.shape
    target, esz = _label_tensor(target, who)
    if rows is None and same_size:
        if tuple(target.shape) != (B, H, W):
            raise NassegError("{}: target {} does not match logits {}".format(who, tuple(target.shape),
                                                                             tuple(logits.shape)))
    elif rows is None and (target.dim() != 3 or target.shape[0] != B or target.numel() == 0):
        raise NassegError("{}: the target must be uint8 or int64 of shape ({}, H, W) (got {})".format(
            who, B, tuple(target.shape)))
    if weight is not None:
        require_device(weight)
        if weight.dtype != torch.float32 or tuple(weight.shape) != (C,):
            raise NassegError("{}: the class weights must be fp32 of shape ({},) (got {} {})".format(
                who, C, weight.dtype, tuple(weight.shape)))
        weight = weight.contiguous()
    return logits, target, esz, weight


def _scalar(like):
    return torch.empty((), device=like.device, dtype=torch.float32)


def _ce_outputs(like, B, H, W):
    """what a cross-entropy forward writes besides its loss: stats = {sum of the kept weights, tau}, counts =
    {k, n_valid, n_kept} (int64) and pixel_loss (B, H, W)"""
    return (_vec(like, 2), torch.empty((3,), device=like.device, dtype=torch.int64),
            torch.empty((B, H, W), device=like.device, dtype=torch.float32))


def _upstream(g):
    return g.to(torch.float32).contiguous().view(1)


class _LogSoftmaxNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        logits, target, esz, _ = _segm_inputs("log_softmax_nll", logits, target, None)
        B, C, H, W = logits.shape
        out = _vec(logits, 2)
        ws = _ws(logits, lib.query("nasseg_ce_workspace"))
        lib.call(_k("nasseg_ce_fwd", logits), ptr(logits), ptr(target), esz, B * H * W, C, int(ignore_index),
                 ptr(out), ptr(ws), current_stream())
        ctx.save_for_backward(logits, target, out)
        ctx.cfg = (esz, int(ignore_index))
        return _own_scalar(out, 0)  # (it may be updated in place; backward reads out[1] only)

    @staticmethod
    def backward(ctx, g):
        logits, target, out = ctx.saved_tensors
        esz, ignore = ctx.cfg
        B, C, H, W = logits.shape
        g = _upstream(g)
        d = torch.empty_like(logits)
        lib.call(_k("nasseg_ce_bwd", logits), ptr(logits), ptr(target), esz, ptr(out), ptr(g), B * H * W, C,
                 ignore, ptr(d), current_stream())
        return d, None, None


def log_softmax_nll(logits, target, ignore_index=255):
    """nn.NLLLoss2d(ignore_index)(nn.LogSoftmax()(logits), target) -> 0-dim tensor."""
    return _LogSoftmaxNLL.apply(logits, target, ignore_index)


class _LogSoftmaxNLLMSE(torch.autograd.Function):
    """(nll, mse) from one nasseg_ce_mse_fwd; backward hands both upstream gradients to one nasseg_ce_mse_bwd.
    The two outputs are scalars of their own, written by the kernel (not views of the statistics it saves):
    the reference's ``loss += kd_coeff * mse`` may modify either one in place."""

    @staticmethod
    def forward(ctx, logits, target, teacher, ignore_index):
        logits, target, esz, _ = _segm_inputs("log_softmax_nll_mse", logits, target, None)
        B, C, H, W = logits.shape
        require_device(teacher)
        if tuple(teacher.shape) != (B, C, H, W) or teacher.dtype != torch.float32:
            raise NassegError("log_softmax_nll_mse: the teacher must be fp32 of the logits' shape {} (got {} {})"
                              .format(tuple(logits.shape), teacher.dtype, tuple(teacher.shape)))
        teacher = teacher.contiguous(memory_format=torch.channels_last)
        nll, mse = _scalar(logits), _scalar(logits)
        stats = _vec(logits, 2)
        ws = _ws(logits, lib.query("nasseg_ce_mse_workspace"))
        lib.call(_k("nasseg_ce_mse_fwd", logits), ptr(logits), ptr(target), esz, ptr(teacher), B * H * W, C,
                 int(ignore_index), ptr(nll), ptr(mse), ptr(stats), ptr(ws), current_stream())
        ctx.save_for_backward(logits, target, teacher, stats)
        ctx.cfg = (esz, int(ignore_index))
        return nll, mse

    @staticmethod
    def backward(ctx, g_nll, g_mse):
        logits, target, teacher, stats = ctx.saved_tensors
        esz, ignore = ctx.cfg
        B, C, H, W = logits.shape
        g_nll, g_mse = _upstream(g_nll), _upstream(g_mse)
        d = torch.empty_like(logits)
        lib.call(_k("nasseg_ce_mse_bwd", logits), ptr(logits), ptr(target), esz, ptr(teacher), ptr(stats),
                 ptr(g_nll), ptr(g_mse), B * H * W, C, ignore, ptr(d), current_stream())
        return d, None, None, None


def log_softmax_nll_mse(logits, target, teacher, ignore_index=255):
    """(nn.NLLLoss2d(ignore_index)(nn.LogSoftmax()(logits), target), nn.MSELoss()(logits, teacher)) -> two 0-dim
    tensors, both differentiable: the decoder-only step's loss and its distillation term (src/engine/trainer.py:
    144-149) from one pass over the logits.  ``teacher``: fp32, the logits' shape (the task0 cache's kd_y)."""
    return _LogSoftmaxNLLMSE.apply(logits, target, teacher, ignore_index)


def _own_scalar(t, index):
    """element ``index`` of the fp32 vector ``t`` under a 0-dim tensor of its own: what a loss node returns.  Not a
    view of ``t`` - a caller may update a loss in place (``loss += aux_weight * aux_loss``, the reference's idiom),
    which autograd refuses on a view made inside a Function - and not a copy (a 4-byte copy node in a recorded step
    cannot be re-created, graph_dag.py).  A node's backward must not read the element it gave away like this."""
    return torch.empty(0, device=t.device, dtype=torch.float32).set_(t.untyped_storage(), t.storage_offset() + index,
                                                                     (), ())


def _select_config(who, thresh, min_kept, keep_fraction):
    """(select, t_loss, min_kept, keep_fraction) of a hard-example selection; ValueError where the definition
    ("Losses") has no meaning"""
    min_kept, keep_fraction = int(min_kept), float(keep_fraction)
    if thresh is not None and not 0.0 < float(thresh) < 1.0:
        raise ValueError("{}: thresh must lie in (0, 1) (got {})".format(who, thresh))
    if not 0.0 <= keep_fraction <= 1.0:
        raise ValueError("{}: keep_fraction must lie in [0, 1] (got {})".format(who, keep_fraction))
    if min_kept < 0:
        raise ValueError("{}: min_kept must not be negative (got {})".format(who, min_kept))
    select = thresh is not None or min_kept > 0 or keep_fraction > 0
    if select and min_kept < 1:
        raise ValueError("{}: hard-example selection needs min_kept >= 1".format(who))
    t_loss = float("inf") if thresh is None else float(np.float32(-np.log(np.float64(thresh))))
    return int(select), t_loss, min_kept, keep_fraction


def _region_config(who, region, smooth=1.0, classes="present", region_weight=1.0):
    """(alpha, beta, smooth, all_classes, region_weight) of a region-overlap term; ValueError where the definition
    ("Losses") has no meaning.  ``region``: "jaccard" | "dice" | ("tversky", alpha, beta)"""
    if isinstance(region, str) and region in ("jaccard", "dice"):
        alpha = beta = 1.0 if region == "jaccard" else 0.5
    elif isinstance(region, (tuple, list)) and len(region) == 3 and region[0] == "tversky":
        try:
            alpha, beta = float(region[1]), float(region[2])
        except (TypeError, ValueError):
            raise ValueError("{}: (\"tversky\", alpha, beta) needs two numbers (got {!r})".format(who, region))
    else:
        raise ValueError("{}: region must be \"jaccard\", \"dice\" or (\"tversky\", alpha, beta) (got {!r})".format(
            who, region))
    smooth, region_weight = float(smooth), float(region_weight)
    if not (alpha >= 0.0 and beta >= 0.0 and alpha + beta > 0.0) or alpha + beta == float("inf"):
        raise ValueError("{}: alpha, beta >= 0 with alpha + beta > 0 expected (got {}, {})".format(who, alpha, beta))
    if not 0.0 <= smooth < float("inf"):
        raise ValueError("{}: smooth must be finite and not negative (got {})".format(who, smooth))
    if classes not in ("present", "all"):
        raise ValueError("{}: classes must be \"present\" or \"all\" (got {!r})".format(who, classes))
    if classes == "all" and smooth == 0.0:
        raise ValueError("{}: classes=\"all\" needs smooth > 0 (an absent class would be 0 / 0)".format(who))
    if region_weight != region_weight or abs(region_weight) == float("inf"):
        raise ValueError("{}: region_weight must be finite (got {})".format(who, region_weight))
    return alpha, beta, smooth, int(classes == "all"), region_weight


def _lovasz_config(who, lovasz_weight=1.0, classes="present"):
    """(lovasz_weight, all_classes) of a Lovasz-Softmax term; ValueError where the definition (INTEGRATION.md,
    "Losses") has no meaning"""
    try:
        lovasz_weight = float(lovasz_weight)
    except (TypeError, ValueError):
        raise ValueError("{}: lovasz_weight must be a number (got {!r})".format(who, lovasz_weight))
    if lovasz_weight != lovasz_weight or abs(lovasz_weight) == float("inf"):
        raise ValueError("{}: lovasz_weight must be finite (got {})".format(who, lovasz_weight))
    if classes not in ("present", "all"):
        raise ValueError("{}: lovasz_classes must be \"present\" or \"all\" (got {!r})".format(who, classes))
    return lovasz_weight, int(classes == "all")


def _segm_config(who, thresh=None, min_kept=0, keep_fraction=0.0, region=None, region_weight=1.0, region_smooth=1.0,
                 region_classes="present", lovasz_weight=None, lovasz_classes="present"):
    """``cross_entropy_select``'s keyword arguments -> (cfg, rcfg, lcfg): the selection, and the region and Lovasz
    terms or None where there is no such term; ValueError as the three functions above raise it"""
    cfg = _select_config(who, thresh, min_kept, keep_fraction)
    rcfg = lcfg = None
    if region is not None:
        rcfg = _region_config(who, region, region_smooth, region_classes, region_weight)
    if lovasz_weight is not None:
        lcfg = _lovasz_config(who, lovasz_weight, lovasz_classes)
    return cfg, rcfg, lcfg


def _lovasz_forward(logits, target, esz, ignore_index, lcfg, base, want_parts):
    """nasseg_lovasz_fwd on checked inputs -> (loss, L_lovasz, errors, G, rank, ncls); the errors and the ranks are
    kept only for ``want_parts`` (the errors are the launch's scratch otherwise, the ranks are not written)"""
    B, C, H, W = logits.shape
    dev = logits.device
    lovasz_weight, all_classes = lcfg
    loss = torch.empty((), device=dev, dtype=torch.float32)
    llov = torch.empty((), device=dev, dtype=torch.float32)
    errors = torch.empty((B, H, W, C), device=dev, dtype=torch.float32)
    coef = torch.empty((B, H, W, C), device=dev, dtype=torch.float32)
    rank = torch.empty((B, H, W, C), device=dev, dtype=torch.int32) if want_parts else None
    ncls = torch.empty((C + 1,), device=dev, dtype=torch.int64)
    ws = _ws(logits, lib.query("nasseg_lovasz_workspace", B * H * W, C))
    lib.call(_k("nasseg_lovasz_fwd", logits), ptr(logits), ptr(target), esz, B * H * W, C, int(ignore_index),
             all_classes, lovasz_weight, ptr(base), ptr(loss), ptr(llov), ptr(errors), ptr(coef), ptr(rank), ptr(ncls),
             ptr(ws), current_stream())
    return loss, llov, (errors if want_parts else None), coef, rank, ncls


def _lovasz_backward(logits, target, esz, ignore, coef, g, lovasz_weight, accumulate, d):
    B, C, H, W = logits.shape
    lib.call(_k("nasseg_lovasz_bwd", logits), ptr(logits), ptr(target), esz, ptr(coef), ptr(g), lovasz_weight,
             int(accumulate), B * H * W, C, ignore, ptr(d), current_stream())
    return d


# What _SegmCriterion returns; a part its terms do not produce is None.  sums = I | S (2C,) and region_ncls = N | |K|
# (C + 1,) int64 are the region term's; errors, rank (B, H, W, C) and lovasz_ncls the Lovasz term's when it runs alone
# and its parts are wanted.
_SegmParts = collections.namedtuple("_SegmParts", "loss pixel_loss tau counts loss_ce loss_region loss_lovasz sums "
                                                  "region_ncls errors rank lovasz_ncls")


class _SegmCriterion(torch.autograd.Function):
    """The composed criterion over logits at the labels' size, one node and one dlogits: the cross-entropy with class
    weights and selection ``cfg`` (nasseg_ce_sel_fwd / _bwd), with the region term ``rcfg`` computed by the same two
    passes (nasseg_ce_region_fwd / _bwd, which also run the region term alone), plus the Lovasz term ``lcfg``:
    nasseg_lovasz_fwd adds it onto the base loss on the device, nasseg_lovasz_bwd adds its gradient onto what the
    base's backward launch has just written (or writes it, alone).  Any of the three may be None, not all.
    Outputs: the fields of _SegmParts - the loss (a scalar of its own: ``loss += aux`` is fine), the others not
    differentiable.  Kept for backward beyond the logits and labels: what the terms present need - pixel_loss and
    stats (cross-entropy), 2C coefficients (region), G, one fp32 [P][C] tensor (Lovasz)."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, cfg, rcfg, lcfg, want_parts):
        with_ce = cfg is not None
        who = "cross_entropy_select" if with_ce else "region_overlap_loss" if rcfg else "lovasz_softmax_loss"
        logits, target, esz, weight = _segm_inputs(who, logits, target, weight)
        B, C, H, W = logits.shape
        ignore = int(ignore_index)
        loss = stats = counts = pixel_loss = tau = loss_ce = loss_region = rcoef = sums = rncls = None
        if with_ce:
            stats, counts, pixel_loss = _ce_outputs(logits, B, H, W)
            tau = _own_scalar(stats, 1)
        if rcfg is not None:
            alpha, beta, smooth, all_classes, region_weight = rcfg
            loss, loss_ce, loss_region = _scalar(logits), _scalar(logits), _scalar(logits)
            rcoef, sums = _vec(logits, 2 * C), _vec(logits, 2 * C)
            rncls = torch.empty((C + 1,), device=logits.device, dtype=torch.int64)
            ws = _ws(logits, lib.query("nasseg_ce_region_workspace", C))
            lib.call(_k("nasseg_ce_region_fwd", logits), ptr(logits), ptr(target), esz, ptr(weight), B * H * W, C,
                     ignore, int(with_ce), *(cfg if with_ce else (0, float("inf"), 0, 0.0)), alpha, beta, smooth,
                     all_classes, region_weight, ptr(loss), ptr(loss_ce), ptr(loss_region), ptr(stats), ptr(counts),
                     ptr(pixel_loss), ptr(rcoef), ptr(sums), ptr(rncls), ptr(ws), current_stream())
        elif with_ce:
            loss = _scalar(logits)
            ws = _ws(logits, lib.query("nasseg_ce_sel_workspace"))
            lib.call(_k("nasseg_ce_sel_fwd", logits), ptr(logits), ptr(target), esz, ptr(weight), B * H * W, C, ignore,
                     *cfg, ptr(loss), ptr(stats), ptr(counts), ptr(pixel_loss), ptr(ws), current_stream())
        llov = lcoef = errors = rank = lncls = None
        if lcfg is not None:
            alone = loss is None  # (no base to add onto: the term's own parts are what there is to return)
            if rcfg is None:
                loss_ce = loss
            loss, llov, errors, lcoef, rank, lncls = _lovasz_forward(logits, target, esz, ignore, lcfg, loss,
                                                                     want_parts and alone)
            if alone:
                llov = None
            if errors is None:
                lncls = None
        ctx.save_for_backward(logits, target, weight, pixel_loss, stats, rcoef, lcoef)
        ctx.cfg = (esz, ignore, with_ce, None if rcfg is None else rcfg[4], None if lcfg is None else lcfg[0])
        outs = _SegmParts(loss, pixel_loss, tau, counts, loss_ce, loss_region, llov, sums, rncls, errors, rank, lncls)
        ctx.mark_non_differentiable(*[o for o in outs[1:] if o is not None])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g, *unused):
        logits, target, weight, pixel_loss, stats, rcoef, lcoef = ctx.saved_tensors
        esz, ignore, with_ce, region_weight, lovasz_weight = ctx.cfg
        B, C, H, W = logits.shape
        g = _upstream(g)
        d = torch.empty_like(logits)
        if rcoef is not None:
            lib.call(_k("nasseg_ce_region_bwd", logits), ptr(logits), ptr(target), esz, ptr(weight), ptr(pixel_loss),
                     ptr(stats), ptr(rcoef), ptr(g), int(with_ce), region_weight, B * H * W, C, ignore, ptr(d),
                     current_stream())
        elif with_ce:
            lib.call(_k("nasseg_ce_sel_bwd", logits), ptr(logits), ptr(target), esz, ptr(weight), ptr(pixel_loss),
                     ptr(stats), ptr(g), B * H * W, C, ignore, ptr(d), current_stream())
        if lcoef is not None:
            _lovasz_backward(logits, target, esz, ignore, lcoef, g, lovasz_weight, with_ce or rcoef is not None, d)
        return (d,) + (None,) * 7


def _segm_criterion(logits, target, weight, ignore_index, cfg, rcfg, lcfg, want_parts=False):
    return _SegmParts(*_SegmCriterion.apply(logits, target, weight, ignore_index, cfg, rcfg, lcfg, bool(want_parts)))


def lovasz_softmax_loss(logits, target, classes="present", ignore_index=255, return_parts=False):
    """Lovasz-Softmax loss (Berman, Triggs, Blaschko, CVPR 2018) of (B, C, H, W) logits -> 0-dim loss of its own
    storage ("Losses"): the Lovasz term of ``cross_entropy_select(lovasz_weight=...)`` alone, bit for
    bit.

    Over the valid pixels (label != ignore_index, in [0, C)), with q = softmax(logits): e_pc = |[t_p == c] - q_pc| in
    fp32; per class the pixels sorted by e descending, ties by ascending pixel index; loss_c = sum_i e_(i) g_i with
    g the Lovasz gradient of the Jaccard loss (in double, from integer counts); loss = mean of loss_c over the classes
    with a pixel (``classes="all"``: over every class); exactly 0 with a zero gradient when no pixel is valid.  The
    order and g are constants in backward.
    ``return_parts``: (loss, errors (B, H, W, C) fp32 with -1 on invalid pixels, rank (B, H, W, C) int32: the 0-based
    position of each valid pixel in its class's order (-1 on invalid pixels and for classes that do not take part),
    N (C,) int64, |K| 0-dim int64).
    The sort runs on the device (a stable radix sort): deterministic, no host synchronisation: capturable."""
    lcfg = _lovasz_config("lovasz_softmax_loss", 1.0, classes)
    out = _segm_criterion(logits, target, None, ignore_index, None, None, lcfg, return_parts)
    if not return_parts:
        return out.loss
    C = out.lovasz_ncls.numel() - 1
    return out.loss, out.errors, out.rank, out.lovasz_ncls[:C], out.lovasz_ncls[C]


def lovasz_from_errors(errors, target, classes="present", ignore_index=255):
    """The sort-and-scan half of ``lovasz_softmax_loss`` over any non-negative fp32 ``errors`` (..., C) with labels
    ``target`` (...) -> (loss 0-dim, coef = G fp32 like ``errors``, rank int32 like ``errors``, N (C,) int64, |K| 0-dim
    int64); not differentiable.  loss = mean over K of sum_i e_(i) g_i, G_pc = -+ g / |K| ("Losses")."""
    _, all_classes = _lovasz_config("lovasz_from_errors", 1.0, classes)
    require_device(errors)
    target, esz = _label_tensor(target)
    if errors.dtype != torch.float32 or errors.dim() < 2 or tuple(errors.shape[:-1]) != tuple(target.shape):
        raise NassegError("lovasz_from_errors: fp32 errors (..., C) and labels (...) expected (got {} {} and {})".format(
            errors.dtype, tuple(errors.shape), tuple(target.shape)))
    errors = errors.detach().contiguous()
    C = errors.shape[-1]
    P = errors.numel() // max(C, 1)
    dev = errors.device
    loss = torch.empty((), device=dev, dtype=torch.float32)
    coef = torch.empty_like(errors)
    rank = torch.empty(errors.shape, device=dev, dtype=torch.int32)
    ncls = torch.empty((C + 1,), device=dev, dtype=torch.int64)
    ws = _ws(errors, lib.query("nasseg_lovasz_workspace", P, C))
    lib.call("nasseg_lovasz_coef", ptr(errors), ptr(target), esz, P, C, int(ignore_index), all_classes, ptr(loss),
             ptr(coef), ptr(rank), ptr(ncls), ptr(ws), current_stream())
    return loss, coef, rank, ncls[:C], ncls[C]


def region_overlap_loss(logits, target, region="jaccard", smooth=1.0, classes="present", ignore_index=255,
                        return_parts=False):
    """Soft Jaccard / Dice / Tversky loss of (B, C, H, W) logits -> 0-dim loss of its own storage (INTEGRATION.md,
    "Losses"): the region term of ``cross_entropy_select(region=...)`` alone, bit for bit.

    Over the valid pixels (label != ignore_index, in [0, C)), with q = softmax(logits): I_c = sum q_c [t == c],
    S_c = sum q_c, N_c = sum [t == c]; T_c = (I_c + smooth) / ((1 - a - b) I_c + a S_c + b N_c + smooth);
    loss = 1 - mean of T_c over the classes with N_c > 0 (``classes="all"``: over every class; needs smooth > 0);
    exactly 0 with a zero gradient when there is no such class.  ``region``: "jaccard" (a = b = 1), "dice"
    (a = b = 0.5) or ("tversky", a, b) with a, b >= 0, a + b > 0.
    ``return_parts``: (loss, I (C,) fp32, S (C,) fp32, N (C,) int64, |K| 0-dim int64).
    Deterministic, no host synchronisation: capturable."""
    rcfg = _region_config("region_overlap_loss", region, smooth, classes)
    out = _segm_criterion(logits, target, None, ignore_index, None, rcfg, None)
    if not return_parts:
        return out.loss
    C = out.sums.numel() // 2
    return out.loss, out.sums[:C], out.sums[C:], out.region_ncls[:C], out.region_ncls[C]


def cross_entropy_select(logits, target, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0,
                         return_parts=False, region=None, region_weight=1.0, region_smooth=1.0,
                         region_classes="present", lovasz_weight=None, lovasz_classes="present"):
    """Class-weighted cross-entropy of (B, C, H, W) logits with online hard-example selection -> 0-dim loss of its
    own storage ("Losses").

    l_p = logsumexp(x_p) - x_p[t] over the valid pixels (label != ignore_index, in [0, C)).  Selection is active iff
    ``thresh`` is given or ``min_kept`` > 0 or ``keep_fraction`` > 0 (then ``min_kept`` >= 1 is required):
    k = min(n_valid, max(min_kept, ceil(keep_fraction * n_valid))), tau = min(-log(thresh), k-th largest l_p), and a
    valid pixel is kept iff l_p >= tau - always on the unweighted l_p.  loss = sum_kept w[t] l_p / sum_kept w[t];
    tau and the kept set are constants in backward, pixels that are not kept get exact zeros.
    ``thresh=0.7, min_kept=100000``: the usual OHEM cross-entropy; ``keep_fraction=0.25`` alone (with min_kept=1):
    top-k bootstrapping; nothing but ``weight``: torch's ``cross_entropy(weight=..., ignore_index=...)``.
    ``return_parts``: (loss, pixel_loss (B, H, W) with -1 on invalid pixels, tau, counts = [k, n_valid, n_kept]).
    ``region`` ("jaccard" | "dice" | ("tversky", a, b); ``region_smooth``, ``region_classes``: the ``smooth`` and
    ``classes`` of ``region_overlap_loss``): loss = the above + ``region_weight`` * that region term over ALL valid
    pixels (selection does not thin it, the weights do not enter it), from the same two passes over the logits;
    ``return_parts`` then also returns the two component losses: (loss, pixel_loss, tau, counts, loss_ce,
    loss_region).
    ``lovasz_weight`` (a number; None: no such term, and nothing here changes): ``lovasz_weight`` *
    ``lovasz_softmax_loss(logits, target, lovasz_classes, ignore_index)`` is added, over ALL valid pixels and without
    the class weights, in the same autograd node; ``return_parts`` then ends with loss_ce (where it was absent) and
    loss_lovasz: (loss, pixel_loss, tau, counts, loss_ce[, loss_region], loss_lovasz).
    No host synchronisation: capturable."""
    cfg, rcfg, lcfg = _segm_config("cross_entropy_select", thresh, min_kept, keep_fraction, region, region_weight,
                                   region_smooth, region_classes, lovasz_weight, lovasz_classes)
    out = _segm_criterion(logits, target, weight, ignore_index, cfg, rcfg, lcfg)
    if not return_parts:
        return out.loss
    parts = (out.loss, out.pixel_loss, out.tau, out.counts)
    if rcfg is not None or lcfg is not None:
        parts += (out.loss_ce,)
    if rcfg is not None:
        parts += (out.loss_region,)
    if lcfg is not None:
        parts += (out.loss_lovasz,)
    return parts


class _CrossEntropyUpsampled(torch.autograd.Function):
    """nasseg_ce_up_fwd / _bwd.  Outputs: the loss (a scalar of its own), and - not differentiable - pixel_loss at the
    labels' size (B, H, W), tau (0-dim) and counts = {k, n_valid, n_kept} (int64).  ``rows`` (or None): the
    row-indexed twins nasseg_ce_up_rows_fwd / _bwd on the label cache ``target`` (_ce_up_entry).
    ``rcfg`` (_region_config's tuple, or None): nasseg_ce_up_region_fwd / _bwd instead - the region-overlap term over
    the label pixels on top (``cfg`` None: alone) - and four more outputs, not differentiable: loss_ce, loss_region,
    sums = I | S (2C,), ncls = N | |K| (C + 1,) int64; tau and counts are then None without the cross-entropy.  Kept
    for backward beyond the plain node's: 2C coefficients and gdot (B, H, W)."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, cfg, rows, rcfg=None):
        with_ce = cfg is not None
        who = "cross_entropy_upsampled" if with_ce else "region_overlap_loss_upsampled"
        logits, target, esz, weight = _segm_inputs(who, logits, target, weight, same_size=False, rows=rows)
        B, C, h, w = logits.shape
        if C < 2:
            raise NassegError("{}: at least two classes are expected (got logits {})".format(who, tuple(logits.shape)))
        H, W = int(target.shape[1]), int(target.shape[2])
        dims = (B, h, w, C, H, W)
        n_ws = lib.query("nasseg_ce_up_workspace" if rcfg is None else "nasseg_ce_up_region_workspace", *dims)
        if n_ws <= 0:
            raise NassegError("{}: logits {} against labels {} exceed B*H*W < 2^32, "
                              "B*h*w*C < 2^31 or 2^24 tiles of 8 x 8 logits and 64 channels".format(
                                  who, tuple(logits.shape), tuple(target.shape)))
        loss = _scalar(logits)
        stats, counts, pixel_loss = _ce_outputs(logits, B, H, W)
        lse = torch.empty((B, H, W), device=logits.device, dtype=torch.float32)
        ws = _ws(logits, n_ws)
        n_rows = None if rows is None else int(target.shape[0])
        ctx.cfg = (esz, int(ignore_index), dims, n_rows, with_ce, None if rcfg is None else rcfg[4])
        if rcfg is None:
            name, table = _ce_up_entry("_fwd", logits, rows, n_rows)
            lib.call(name, ptr(logits), ptr(target), esz, *table, ptr(weight), *dims, int(ignore_index), *cfg,
                     ptr(loss), ptr(stats), ptr(counts), ptr(pixel_loss), ptr(lse), ptr(ws), current_stream())
            ctx.save_for_backward(logits, target, weight, pixel_loss, lse, stats, rows)
            tau = _own_scalar(stats, 1)
            ctx.mark_non_differentiable(pixel_loss, tau, counts)
            return loss, pixel_loss, tau, counts
        alpha, beta, smooth, all_classes, region_weight = rcfg
        loss_ce, loss_region = _scalar(logits), _scalar(logits)
        rcoef, sums = _vec(logits, 2 * C), _vec(logits, 2 * C)
        ncls = torch.empty((C + 1,), device=logits.device, dtype=torch.int64)
        gdot = torch.empty((B, H, W), device=logits.device, dtype=torch.float32)
        if not with_ce:
            stats = counts = None
        name, table = _ce_up_entry("_fwd", logits, rows, n_rows, region=True)
        lib.call(name, ptr(logits), ptr(target), esz, *table, ptr(weight), *dims, int(ignore_index), int(with_ce),
                 *(cfg if with_ce else (0, float("inf"), 0, 0.0)), alpha, beta, smooth, all_classes, region_weight,
                 ptr(loss), ptr(loss_ce), ptr(loss_region), ptr(stats), ptr(counts), ptr(pixel_loss), ptr(lse),
                 ptr(rcoef), ptr(sums), ptr(ncls), ptr(gdot), ptr(ws), current_stream())
        ctx.save_for_backward(logits, target, weight, pixel_loss, lse, stats, rows, rcoef, gdot)
        tau = _own_scalar(stats, 1) if with_ce else None
        outs = (loss, pixel_loss, tau, counts, loss_ce, loss_region, sums, ncls)
        ctx.mark_non_differentiable(*[o for o in outs[1:] if o is not None])
        return outs

    @staticmethod
    def backward(ctx, g, *unused):
        esz, ignore, dims, n_rows, with_ce, region_weight = ctx.cfg
        g = _upstream(g)
        if region_weight is None:
            logits, target, weight, pixel_loss, lse, stats, rows = ctx.saved_tensors
            d = torch.empty_like(logits)
            name, table = _ce_up_entry("_bwd", logits, rows, n_rows)
            lib.call(name, ptr(logits), ptr(target), esz, *table, ptr(weight), ptr(pixel_loss), ptr(lse), ptr(stats),
                     ptr(g), *dims, ignore, ptr(d), current_stream())
        else:
            logits, target, weight, pixel_loss, lse, stats, rows, rcoef, gdot = ctx.saved_tensors
            d = torch.empty_like(logits)
            name, table = _ce_up_entry("_bwd", logits, rows, n_rows, region=True)
            lib.call(name, ptr(logits), ptr(target), esz, *table, ptr(weight), ptr(pixel_loss), ptr(lse), ptr(stats),
                     ptr(rcoef), ptr(gdot), ptr(g), int(with_ce), region_weight, *dims, ignore, ptr(d),
                     current_stream())
        return d, None, None, None, None, None, None


def _ce_up_entry(end, logits, rows, n_rows, region=False):
    """(entry point, the arguments that follow elem_size) of the full-size cross-entropy's ``end`` ("_fwd" | "_bwd")
    for logits stored like ``logits``: with ``rows`` the row-indexed twin and its table (rows, N), without them the
    plain entry point and nothing (as _depth_entry).  ``region``: the entry points with the region-overlap term."""
    base = "nasseg_ce_up_region" if region else "nasseg_ce_up"
    if rows is None:
        return _k(base + end, logits), ()
    return _k(base + "_rows" + end, logits), (ptr(rows), n_rows)


def region_overlap_loss_upsampled(logits, target, region="jaccard", smooth=1.0, classes="present", ignore_index=255,
                                  return_parts=False, rows=None):
    """``region_overlap_loss`` taken at the LABELS' size: the soft Jaccard / Dice / Tversky loss of (B, C, h, w)
    logits up-sampled bilinearly (align_corners=False) to the (B, H, W) labels inside the kernels -> 0-dim loss of its
    own storage ("Losses"): the region term of ``cross_entropy_upsampled(region=...)`` alone.

    ``region``, ``smooth``, ``classes`` and the ``ValueError``s are ``region_overlap_loss``'s; the sums run over the
    valid label pixels with q = exp(v - logsumexp(v)) of the interpolated row v.  Nothing of B*H*W*C elements is
    allocated in either direction.  ``return_parts``: (loss, I (C,) fp32, S (C,) fp32, N (C,) int64, |K| 0-dim int64).
    ``rows``: as ``cross_entropy_upsampled``'s.  Deterministic, no host synchronisation: capturable."""
    rcfg = _region_config("region_overlap_loss_upsampled", region, smooth, classes)
    out = _CrossEntropyUpsampled.apply(logits, target, None, ignore_index, None, rows, rcfg)
    if not return_parts:
        return out[0]
    sums, ncls = out[6], out[7]
    C = sums.numel() // 2
    return out[0], sums[:C], sums[C:], ncls[:C], ncls[C]


def cross_entropy_upsampled(logits, target, weight=None, ignore_index=255, thresh=None, min_kept=0,
                            keep_fraction=0.0, return_parts=False, rows=None, region=None, region_weight=1.0,
                            region_smooth=1.0, region_classes="present"):
    """``cross_entropy_select`` taken at the LABELS' size: the cross-entropy of (B, C, h, w) logits, up-sampled
    bilinearly (align_corners=False) to the (B, H, W) labels inside the kernels -> 0-dim loss of its own storage
    ("Losses").

    The labels may be larger than, equal to or smaller than the logits, per axis; equal sizes give
    ``cross_entropy_select``'s per-pixel losses bit for bit.  The row the loss sees at a label pixel is the row
    ``argmax_confusion`` takes its argmax of in validation.  Class weights, ``ignore_index``, ``thresh`` /
    ``min_kept`` / ``keep_fraction`` (over the B*H*W label pixels) and the ``ValueError``s are those of
    ``cross_entropy_select``.  Nothing of B*H*W*C elements is allocated in either direction: per label pixel the
    loss and the log-sum-exp are kept, the gradient is gathered straight into the logits' shape (exact zeros where
    no kept label pixel reaches a logit).
    ``return_parts``: (loss, pixel_loss (B, H, W) with -1 on invalid pixels, tau, counts = [k, n_valid, n_kept]).
    No host synchronisation: capturable.
    ``rows`` (a contiguous 1-D int64 device tensor of B entries): ``target`` is a label cache (N, H, W), uint8 or
    int64 and contiguous, and image b meets ``target[rows[b]]`` - read in place by the kernels, bit for bit the call
    on the gathered ``target[rows]``, which is never made (the task0 cache's ``'y_full'``, engine/trainer.py).
    Repeated and unordered rows are legal; B*H*W < 2^32 bounds the batch, the cache may be larger.
    ``region`` ("jaccard" | "dice" | ("tversky", a, b); ``region_smooth``, ``region_classes``: the ``smooth`` and
    ``classes`` of ``region_overlap_loss``; None: no such term, and nothing here changes): loss = the above +
    ``region_weight`` * that region term over ALL valid label pixels (selection does not thin it, the weights do not
    enter it), with q = exp(v - logsumexp(v)) of the interpolated row - the differentiable form of the mean IoU at the
    size ``validate`` measures it.  Still nothing of B*H*W*C elements: one more fp32 value per label pixel is kept.
    ``return_parts`` then also returns the two component losses: (loss, pixel_loss, tau, counts, loss_ce,
    loss_region).  With ``rows`` as well."""
    cfg = _select_config("cross_entropy_upsampled", thresh, min_kept, keep_fraction)
    if region is None:
        out = _CrossEntropyUpsampled.apply(logits, target, weight, ignore_index, cfg, rows, None)
        return out if return_parts else out[0]
    rcfg = _region_config("cross_entropy_upsampled", region, region_smooth, region_classes, region_weight)
    out = _CrossEntropyUpsampled.apply(logits, target, weight, ignore_index, cfg, rows, rcfg)
    return out[:6] if return_parts else out[0]


def ohem_threshold(pixel_loss, thresh=None, min_kept=1, keep_fraction=0.0, t_loss=None):
    """The selection of ``cross_entropy_select`` alone, over any fp32 tensor: entries < 0 do not take part.
    Returns (tau, counts): tau = min(t_loss, k-th largest entry) as a 0-dim fp32 tensor, counts = int64
    [k, n (entries that take part), entries >= tau among them]; t_loss = float32(-log(thresh)), +inf without
    ``thresh`` (``t_loss``: that value given directly).  Exact (a radix select on the device), deterministic, no
    host synchronisation."""
    require_device(pixel_loss)
    if pixel_loss.dtype != torch.float32 or pixel_loss.numel() == 0:
        raise NassegError("ohem_threshold: a non-empty fp32 tensor is expected (got {} {})".format(
            pixel_loss.dtype, tuple(pixel_loss.shape)))
    _, t, min_kept, keep_fraction = _select_config("ohem_threshold", thresh, min_kept, keep_fraction)
    if t_loss is not None:
        if thresh is not None:
            raise ValueError("ohem_threshold: give thresh or t_loss, not both")
        t = float(t_loss)
    v = pixel_loss.contiguous()
    tau = torch.empty((), device=v.device, dtype=torch.float32)
    counts = torch.empty((3,), device=v.device, dtype=torch.int64)
    ws = _ws(v, lib.query("nasseg_ohem_workspace"))
    lib.call("nasseg_ohem_threshold", ptr(v), v.numel(), t, min_kept, keep_fraction, ptr(tau), ptr(counts), ptr(ws),
             current_stream())
    return tau, counts


class _BerHu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        require_device(pred, target)
        if pred.dtype not in (torch.float32, torch.bfloat16) or target.dtype != pred.dtype:
            raise NassegError("berhu: fp32 or bf16 tensors of one dtype expected")
        if pred.shape != target.shape:
            raise NassegError("berhu: shapes differ")
        p, t = pred.contiguous(), target.contiguous()
        out = _vec(p, 2)
        ws = _ws(p, lib.query("nasseg_ce_workspace"))
        lib.call(_k("nasseg_berhu_fwd", p), ptr(p), ptr(t), p.numel(), ptr(out), ptr(ws), current_stream())
        ctx.save_for_backward(p, t, out)
        return _own_scalar(out, 0)  # (it may be updated in place; backward reads c = out[1] only)

    @staticmethod
    def backward(ctx, g):
        p, t, out = ctx.saved_tensors
        g = _upstream(g)
        d = torch.empty_like(p)
        lib.call(_k("nasseg_berhu_bwd", p), ptr(p), ptr(t), ptr(out), ptr(g), p.numel(), ptr(d),
                 current_stream())
        return d, None


def berhu_loss(pred, target):
    """Reverse-Huber loss of the depth head (absent from the reference; oracle/losses.py)."""
    return _BerHu.apply(pred, target)


def _depth_inputs(who, pred, target, rows):
    """(p, t, rows, n_rows, (B, h, w, H, W)) as the depth losses' kernels read them: a contiguous prediction
    (B, 1, h, w), fp32 or bf16, and a contiguous fp32 target (B, H, W) of any size.  ``who``: the public function the
    user called, named by every error.
    With ``rows`` the target is a cache (N, H, W), fp32 and contiguous as it stands - it is never copied -, ``rows``
    an int64 device tensor of one cache row per image of ``pred``, and n_rows = N (None without).  An index that can be
    read without a synchronisation (a host tensor) is checked against [0, N) before it is refused for being on the
    host; on the device the kernels clamp (a memory-safety net, as in ``gather_rows``)."""
    n_rows = None
    if rows is not None:
        if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous():
            raise NassegError("{}: rows must be a contiguous 1-D int64 tensor".format(who))
        if not torch.is_tensor(target) or target.dtype != torch.float32 or target.dim() != 3 or target.shape[0] < 1:
            raise NassegError("{}: with rows, the target must be an fp32 cache of shape (N, H, W) (got {} {})".format(
                who, getattr(target, "dtype", None), tuple(getattr(target, "shape", ()))))
        n_rows = int(target.shape[0])
        if rows.shape[0] != pred.shape[0]:
            raise NassegError("{}: one cache row per image expected ({} rows for {} images)".format(
                who, rows.shape[0], pred.shape[0]))
        if not rows.is_cuda and rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n_rows):
            raise IndexError("{}: cache row index out of range [0, {})".format(who, n_rows))
    require_device(pred, target, rows)
    if rows is not None and not target.is_contiguous():
        raise NassegError("{}: with rows, the target cache must be contiguous (it is read in place)".format(who))
    if pred.dtype not in (torch.float32, torch.bfloat16) or pred.dim() != 4 or pred.shape[1] != 1:
        raise NassegError("{}: the prediction must be fp32 or bf16 of shape (B, 1, h, w) (got {} {})".format(
            who, pred.dtype, tuple(pred.shape)))
    if target.dtype != torch.float32 or target.dim() != 3 or (rows is None and target.shape[0] != pred.shape[0]):
        raise NassegError("{}: the target must be fp32 of shape (B, H, W) (got {} {})".format(
            who, target.dtype, tuple(target.shape)))
    p, t = pred.contiguous(), target.contiguous()  # (one channel: NCHW and NHWC are the same memory)
    B, _, h, w = p.shape
    return p, t, rows, n_rows, (B, h, w, int(t.shape[1]), int(t.shape[2]))


def _depth_entry(base, end, p, rows, n_rows):
    """(entry point, the arguments that follow ptr(t)) of the depth loss ``base`` + ``end`` ("_fwd" | "_bwd") for a
    prediction stored like ``p``: with ``rows`` the row-indexed twin ``base``_rows``end`` and its table (rows, N),
    without them the plain entry point and nothing"""
    if rows is None:
        return _k(base + end, p), ()
    return _k(base + "_rows" + end, p), (ptr(rows), n_rows)


# What _DepthCriterion returns; a part its combination does not produce is None.  berhu, silog (D) and grad_match
# (L_gm) are the terms'; c is the berHu's threshold when it runs alone.
_DepthParts = collections.namedtuple("_DepthParts", "loss berhu c n_valid silog grad_match")


class _DepthCriterion(torch.autograd.Function):
    """The depth criterion against a full-size target with holes, one node and one dpred.  ``sampling`` "masked": the
    target sampled (nearest) at the prediction's size, nasseg_berhu_masked_fwd / _bwd; with ``terms``
    (_depth_terms_config's tuple, else None) nasseg_depth_terms_fwd adds the scale-invariant and gradient-matching
    terms to that berHu and nasseg_depth_terms_bwd writes the gradient of all three.  "up": the prediction up-sampled
    bilinearly to the target's size, nasseg_berhu_up_fwd / _bwd, ``group`` the backward's lanes per prediction pixel
    (0: from the shapes); the library has no terms there.  ``rows`` (or None): the row-indexed twins of the same entry
    points on the cache ``target`` (_depth_entry).
    Outputs: the fields of _DepthParts, 0-dim fp32 scalars of their own on the kernels' output vectors - the loss may
    be updated in place, the others are not differentiable.  Kept for backward: p, t, the berHu's
    {loss, c, n_valid} and rows, with the terms also their residuals and 16 floats."""

    @staticmethod
    def forward(ctx, pred, target, valid_min, valid_max, sampling, group, terms, rows):
        up = sampling == "up"
        who = "depth_criterion" if terms is not None else "berhu_loss_upsampled" if up else "berhu_loss_masked"
        if sampling not in ("masked", "up") or (up and terms is not None):
            raise NassegError("depth_criterion: sampling is \"masked\" or \"up\" (got {!r}), and the scale-invariant "
                              "and gradient-matching terms are defined at the prediction's size only".format(sampling))
        p, t, rows, n_rows, dims = _depth_inputs(who, pred, target, rows)
        if up:
            base, n_ws = "nasseg_berhu_up", lib.query("nasseg_berhu_up_workspace", *dims)
            if n_ws <= 0:
                raise NassegError("berhu_loss_upsampled: prediction {} against target {} is empty or exceeds "
                                  "B*H*W < 2^32, B*h*w < 2^31".format(tuple(pred.shape), tuple(target.shape)))
        else:
            base, n_ws = "nasseg_berhu_masked", lib.query("nasseg_berhu_masked_workspace")
        geom = dims + (float(valid_min), float(valid_max))
        stats, ws = _vec(p, 3), _ws(p, n_ws)
        name, table = _depth_entry(base, "_fwd", p, rows, n_rows)
        lib.call(name, ptr(p), ptr(t), *table, *geom, ptr(stats), ptr(ws), current_stream())
        resid = out = None
        if terms is None:
            cfg = geom + ((int(group),) if up else ())
            parts = _DepthParts(_own_scalar(stats, 0), None, _own_scalar(stats, 1), _own_scalar(stats, 2), None, None)
        else:
            bw, sw, lam, gw, scales, pmin = terms
            base, cfg = "nasseg_depth_terms", geom + (pmin, lam, scales, bw, sw, gw)
            resid, out = torch.empty(dims[:3], device=p.device, dtype=torch.float32), _vec(p, 16)
            ws = _ws(p, lib.query("nasseg_depth_terms_workspace"))
            name, table = _depth_entry(base, "_fwd", p, rows, n_rows)
            lib.call(name, ptr(p), ptr(t), *table, *geom, pmin, lam, scales, ptr(stats), bw, sw, gw, ptr(resid),
                     ptr(out), ptr(ws), current_stream())
            parts = _DepthParts(_own_scalar(out, 0), _own_scalar(stats, 0), None, _own_scalar(out, 3),
                                _own_scalar(out, 1), _own_scalar(out, 2))
        ctx.save_for_backward(p, t, stats, rows, resid, out)
        ctx.cfg = (base, n_rows, cfg)  # (base: the backward's entry point)
        ctx.mark_non_differentiable(*[o for o in parts[1:] if o is not None])
        ctx.set_materialize_grads(False)  # (no zero-fill launch per part that backward ignores)
        return tuple(parts)

    @staticmethod
    def backward(ctx, g, *unused):
        p, t, stats, rows, resid, out = ctx.saved_tensors
        base, n_rows, cfg = ctx.cfg
        g = _upstream(g)
        d = torch.empty_like(p)
        name, table = _depth_entry(base, "_bwd", p, rows, n_rows)
        kept = (ptr(stats),) if out is None else (ptr(resid), ptr(stats), ptr(out))
        lib.call(name, ptr(p), ptr(t), *table, *kept, ptr(g), *cfg, ptr(d), current_stream())
        return (d,) + (None,) * 7


def _depth_criterion(pred, target, valid_min, valid_max, sampling="masked", group=0, terms=None, rows=None):
    return _DepthParts(*_DepthCriterion.apply(pred, target, valid_min, valid_max, sampling, group, terms, rows))


def berhu_loss_masked(pred, target, valid_min=0.0, valid_max=float("inf"), rows=None):
    """Reverse-Huber loss of a depth head against a full-size target with holes (absent from the reference).

    pred (B, 1, h, w) fp32 or bf16, target (B, H, W) fp32 at ANY size: prediction pixel (y, x) is compared with the
    target pixel ``F.interpolate(mode="nearest")`` would put there (never written anywhere).  A pixel counts iff its
    target t is finite and ``valid_min < t <= valid_max``; d = |pred - t|, c = 0.2 * max d (a constant in backward),
    loss = mean over valid pixels of (d if d <= c else (d^2 + c^2) / (2c)); no valid pixel: loss 0, gradient 0.
    Returns a 0-dim tensor that may be updated in place.  No host synchronisation: capturable.
    ``rows`` (an int64 device tensor of B entries): ``target`` is a cache (N, H, W), fp32 and contiguous, and image b
    meets ``target[rows[b]]`` - read in place by the kernels, bit for bit the call on the gathered ``target[rows]``,
    which is never made (the task0 depth cache, engine/trainer.py).  Repeated and unordered rows are legal."""
    return _depth_criterion(pred, target, valid_min, valid_max, rows=rows).loss


def berhu_loss_upsampled(pred, target, valid_min=0.0, valid_max=float("inf"), return_parts=False, rows=None):
    """``berhu_loss_masked`` taken at the TARGET's size: the reverse-Huber loss of a depth head whose prediction is
    up-sampled bilinearly (align_corners=False) to the (B, H, W) target inside the kernels ("Depth").

    pred (B, 1, h, w) fp32 or bf16, target (B, H, W) fp32 at ANY size, larger than, equal to or smaller than the
    prediction, per axis.  A TARGET pixel counts iff it is finite and ``valid_min < t <= valid_max``; v = the
    up-sampled prediction there - the value ``depth_metrics`` scores, bit for bit; d = |v - t|, c = 0.2 * max d (a
    constant in backward), loss = mean over the valid target pixels of (d if d <= c else (d^2 + c^2) / (2c)); no
    valid pixel: loss 0, gradient 0.  Nothing of the target's size is allocated in either direction: the gradient is
    gathered straight into the prediction's shape (exact zeros where no valid target pixel reaches a prediction
    pixel), without atomics - the same inputs give the same bits.
    Returns a 0-dim tensor that may be updated in place; ``return_parts``: (loss, c, n_valid), all 0-dim fp32.
    No host synchronisation: capturable.
    ``rows``: as in ``berhu_loss_masked`` - ``target`` is a cache (N, H, W) read in place through the B cache rows;
    B*H*W < 2^32 bounds the batch, the cache may be larger."""
    out = _depth_criterion(pred, target, valid_min, valid_max, "up", rows=rows)
    return (out.loss, out.c, out.n_valid) if return_parts else out.loss


def _depth_terms_config(who, valid_min, berhu_weight, silog_weight, silog_lambda, grad_weight, grad_scales, pred_min):
    """(berhu_weight, silog_weight, silog_lambda, grad_weight, scales, pred_min) as the kernels take them - a term
    that is None has weight 0, and without a gradient-matching term scales is 0 (its pass is not launched);
    ValueError where the definition (include/nasseg.h, "Depth terms") has no meaning"""
    def weight(name, v):
        v = float(v)
        if not 0.0 <= v < float("inf"):
            raise ValueError("{}: {} must be a finite number >= 0 (got {})".format(who, name, v))
        return v

    bw = weight("berhu_weight", berhu_weight)
    sw = 0.0 if silog_weight is None else weight("silog_weight", silog_weight)
    gw = 0.0 if grad_weight is None else weight("grad_weight", grad_weight)
    lam, pmin = float(silog_lambda), float(pred_min)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("{}: silog_lambda must lie in [0, 1] (got {})".format(who, silog_lambda))
    if isinstance(grad_scales, bool) or int(grad_scales) != grad_scales or not 1 <= int(grad_scales) <= 8:
        raise ValueError("{}: grad_scales must be an integer in [1, 8] (got {!r})".format(who, grad_scales))
    if not 0.0 < pmin < float("inf"):
        raise ValueError("{}: pred_min must be a finite number > 0 (got {})".format(who, pred_min))
    if not float(valid_min) >= 0.0:
        raise ValueError("{}: the scale-invariant and gradient-matching terms take logarithms of the valid targets: "
                         "valid_min >= 0 is required (got {})".format(who, valid_min))
    return bw, sw, lam, gw, (0 if grad_weight is None else int(grad_scales)), pmin


def depth_criterion(pred, target, valid_min=0.0, valid_max=float("inf"), berhu_weight=1.0, silog_weight=None,
                    silog_lambda=0.5, grad_weight=None, grad_scales=4, pred_min=1e-3, rows=None, return_parts=False):
    """The depth criterion that matches the depth score: ``berhu_weight * berHu + silog_weight * D + grad_weight *
    L_gm`` of a depth head against a full-size target with holes (absent from the reference; definition:
    include/nasseg.h, "Depth terms"; INTEGRATION.md, "Depth").

    pred (B, 1, h, w) fp32 or bf16, target (B, H, W) fp32 at ANY size; sampling and validity are
    ``berhu_loss_masked``'s (nearest sampling of the target at the prediction's size; a pixel counts iff its target t
    is finite and ``valid_min < t <= valid_max``).  With r = ln max(p, pred_min) - ln t over the n valid pixels:
    D = mean(r^2) - silog_lambda * mean(r)^2 is the scale-invariant log term (Eigen et al. 2014, eq. 4) - the
    ``silog`` score of ``validate_depth`` is sqrt(D) at silog_lambda = 1; the root is left out so that the gradient
    stays finite at a perfect prediction.  L_gm = sum over k < grad_scales of (sum over the pixels of the grid with
    stride s = 2^k of |r_right - r| + |r_below - r|, neighbours at distance s inside the image, both ends valid) /
    (valid pixels of that grid) is the multi-scale gradient-matching term (MegaDepth, MiDaS): it rewards sharp depth
    edges.  A term whose weight is None is left out.  A pixel with p <= pred_min gets no gradient from the two terms -
    they sit on top of the berHu, which still pulls such a pixel up.  No valid pixel: loss 0, gradient 0.
    ``valid_min >= 0``, ``pred_min > 0``, ``0 <= silog_lambda <= 1``, ``1 <= grad_scales <= 8`` and weights >= 0:
    anything else is a ValueError.  One autograd node; the backward is one kernel that writes the gradient of all
    three terms once.  Returns a 0-dim tensor that may be updated in place; ``return_parts``: (loss, berhu, D, L_gm,
    n_valid), all 0-dim fp32, the last four not differentiable.  No host synchronisation: capturable; the same
    inputs give the same bits.  ``rows``: as in ``berhu_loss_masked``."""
    terms = _depth_terms_config("depth_criterion", valid_min, berhu_weight, silog_weight, silog_lambda, grad_weight,
                                grad_scales, pred_min)
    out = _depth_criterion(pred, target, valid_min, valid_max, terms=terms, rows=rows)
    return (out.loss, out.berhu, out.silog, out.grad_match, out.n_valid) if return_parts else out.loss


def depth_metrics(pred, gt, min_depth=1e-3, max_depth=10.0, acc=None):
    """Fused bilinear up-sampling -> validity mask -> clamp -> sums of the depth scores: the depth counterpart of
    ``argmax_confusion``.

    pred (B, C, h, w) fp32 or bf16 on the device (channel 0 is the depth; more channels need no copy), gt (B, H, W)
    fp32 on the device.  Pixels whose gt is finite and in (min_depth, max_depth] count; the up-sampled prediction is
    clamped to [min_depth, max_depth].  ``acc`` is a float64 (12,) device tensor that is accumulated into (created
    zeroed when None): n, sum|p-g|, sum(p-g)^2, sum|p-g|/g, sum(p-g)^2/g, sum|log10 p - log10 g|, sum(ln p - ln g),
    sum(ln p - ln g)^2, #{max(p/g, g/p) < 1.25, 1.25^2, 1.25^3}, one reserved slot.
    engine.inference.depth_scores turns it into the scores."""
    pred = _cl(pred.detach())
    require_device(gt)
    B, C, h, w = pred.shape
    if gt.dtype != torch.float32 or gt.dim() != 3 or gt.shape[0] != B:
        raise NassegError("depth_metrics: gt must be fp32 of shape (B, H, W) (got {} {})".format(
            gt.dtype, tuple(gt.shape)))
    gt = gt.contiguous()
    H, W = gt.shape[1], gt.shape[2]
    if acc is None:
        acc = torch.zeros((12,), device=pred.device, dtype=torch.float64)
    elif (tuple(acc.shape) != (12,) or acc.dtype != torch.float64 or not acc.is_contiguous()
          or acc.device != pred.device):
        raise NassegError("depth_metrics: acc must be a contiguous float64 (12,) tensor on the prediction's device")
    ws = torch.empty((max(lib.query("nasseg_depth_metrics_workspace", B, H, W), 1),), device=pred.device,
                     dtype=torch.float64)
    lib.call(_k("nasseg_depth_metrics", pred), ptr(pred), C, B, h, w, ptr(gt), H, W, float(min_depth),
             float(max_depth), ptr(acc), ptr(ws), current_stream())
    return acc


def nearest_label_resize(target, size, out=None):
    """F.interpolate(target[:, None].float(), size, mode='nearest').long()[:, 0]; ``out``: a
    contiguous int64 (B, Ho, Wo) tensor to write into (a slice of the task0 label cache)."""
    target, esz = _label_tensor(target)
    B, H, W = target.shape
    Ho, Wo = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((B, Ho, Wo), device=target.device, dtype=torch.int64)
    elif (tuple(out.shape) != (B, Ho, Wo) or out.dtype != torch.int64 or not out.is_contiguous()
          or out.device != target.device):
        raise NassegError("nearest_label_resize: bad output tensor")
    lib.call("nasseg_nearest_label", ptr(target), esz, ptr(out), B, H, W, Ho, Wo, current_stream())
    return out


def copy_into(dst, src):
    """dst[...] = src for two densely stored activations of one shape and dtype (a slice of the
    task0 cache receiving an encoder output): one copy kernel on the current stream."""
    require_device(dst, src)
    if tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
        raise NassegError("copy_into: shapes / dtypes differ")
    src = src.contiguous(memory_format=torch.channels_last) if src.dim() == 4 else src.contiguous()
    C = src.shape[1] if src.dim() == 4 else 0
    if (src.dim() == 4 and C % 4 == 0 and src.dtype in (torch.float32, torch.bfloat16)
            and dst.is_contiguous(memory_format=torch.channels_last)):
        lib.call(_k("nasseg_chan_copy", src), ptr(src), C, 0, ptr(dst), C, 0, None, 0, 0,
                 src.numel() // C, C, ACT_NONE, ACT_NONE, current_stream())
    else:
        dst.copy_(src)  # (3-channel or integer maps: a plain device copy)
    return dst


def gather_rows(src, idx, out=None):
    """src[idx] along dim 0 for a densely stored tensor (NCHW-contiguous or channels_last: one
    sample = one contiguous row) with an int64 DEVICE index: the batch of the task0 feature cache,
    one copy kernel, no ATen indexing and no layout change (src/engine/trainer.py:128-137)."""
    require_device(src, idx)
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise NassegError("gather_rows: the index must be a contiguous 1-D int64 tensor")
    n = idx.shape[0]
    cl = src.dim() == 4 and src.is_contiguous(memory_format=torch.channels_last)
    if not (cl or src.is_contiguous()):
        raise NassegError("gather_rows: the source must be stored densely")
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), device=src.device, dtype=src.dtype,
                          memory_format=torch.channels_last if cl else torch.contiguous_format)
    row_bytes = (src.numel() // max(src.shape[0], 1)) * src.element_size()
    lib.call("nasseg_gather_rows", ptr(src), ptr(idx), ptr(out), n, row_bytes, src.shape[0], current_stream())
    return out


def _augment(who, src, desc, taps, lut, Ho, Wo, colour=None, depth=None):
    """The body of the four functions below (``who``: the one that called, for its errors).  ``colour``: (colour, ctab)
    of a batch with a ColourJitter; ``depth``: (params, depth_scale) of a depth batch.  The packed batch of
    data/device.py is checked, the image and the target - uint8 labels, fp32 metres for a depth batch - are allocated
    and the entry point of colour x depth is launched once, its arguments in include/nasseg.h's order."""
    jitter, ctab = colour or (None, None)
    params, depth_scale = depth or (None, None)
    require_device(src, desc, taps, jitter, ctab, lut, params)
    B = desc.shape[0] if desc.dim() == 2 else 0
    if (src.dtype != torch.uint8 or desc.dtype != torch.int64 or taps.dtype != torch.int32
            or lut.dtype not in (torch.float32, torch.bfloat16) or src.dim() != 1 or B == 0
            or tuple(desc.shape) != (B, 8) or tuple(taps.shape) != (B, 9 * (Ho + Wo)) or tuple(lut.shape) != (3, 256)
            or not all(t.is_contiguous() for t in (src, desc, taps, lut))
            or (depth and (params.dtype != torch.float32 or tuple(params.shape) != (B, 2)
                           or not params.is_contiguous()))):
        raise NassegError("{}: bad packed batch".format(who))
    if colour and (jitter.dtype != torch.int32 or tuple(jitter.shape) != (B, 12) or not jitter.is_contiguous()
                   or ctab.dtype != torch.uint8 or tuple(ctab.shape) != (B, 3, 256) or not ctab.is_contiguous()
                   or ctab.data_ptr() % 4 != 0):
        raise NassegError("{}: colour must be contiguous int32 [B][12] and ctab contiguous uint8 [B][3][256]".format(
            who))
    image = torch.empty((B, 3, Ho, Wo), device=src.device, dtype=lut.dtype, memory_format=torch.channels_last)
    target = torch.empty((B, Ho, Wo), device=src.device, dtype=torch.float32 if depth else torch.uint8)
    name = "nasseg_augment" + ("_depth" if depth else "") + ("_colour" if colour else "")
    lib.call(_k(name, lut), ptr(src), src.numel(), ptr(desc), ptr(taps),
             *((ptr(jitter), ptr(ctab)) if colour else ()), ptr(lut),
             *((ptr(params), float(depth_scale)) if depth else ()), ptr(image), ptr(target), B, Ho, Wo,
             current_stream())
    return image, target


def augment(src, desc, taps, lut, Ho, Wo):
    """The sample pipelines of data/datasets.py for one packed batch (data/device.py plans and packs it): uint8
    ``src`` (the source windows), int64 ``desc`` [B][8], int32 ``taps`` [B][9 (Ho + Wo)] and the Normalise table
    ``lut`` [3][256] of the output dtype (fp32 or bf16) -> (image B x 3 x Ho x Wo channels_last, mask uint8
    B x Ho x Wo); one nasseg_augment launch (include/nasseg.h)."""
    return _augment("augment", src, desc, taps, lut, Ho, Wo)


def augment_depth(src, desc, taps, lut, params, depth_scale, Ho, Wo):
    """``augment`` for a metric depth target: the "mask" windows of ``src`` hold little-endian 16-bit counts (row
    stride in bytes), fp32 ``params`` [B][2] = {zoom, fill} per sample, ``depth_scale`` metres per count -> (image
    B x 3 x Ho x Wo channels_last of the table's dtype - ``augment``'s, bit for bit -, target fp32 B x Ho x Wo =
    count * depth_scale / zoom in correctly rounded fp32, or the fill undivided); one nasseg_augment_depth launch
    (include/nasseg.h)."""
    return _augment("augment_depth", src, desc, taps, lut, Ho, Wo, depth=(params, depth_scale))


def augment_colour(src, desc, taps, colour, ctab, lut, Ho, Wo):
    """``augment`` with a ColourJitter (data/datasets.py) between the resampling and ``lut``: int32 ``colour``
    [B][12] (the sample's 12-bit colour matrix row-major, 1 / 0: apply it, two zeros) and uint8 ``ctab`` [B][3][256]
    (its point table per channel); fill pixels skip both.  One nasseg_augment_colour launch (include/nasseg.h)."""
    return _augment("augment_colour", src, desc, taps, lut, Ho, Wo, colour=(colour, ctab))


def augment_depth_colour(src, desc, taps, colour, ctab, lut, params, depth_scale, Ho, Wo):
    """``augment_depth`` with ``augment_colour``'s jitter of the image; the target is ``augment_depth``'s.  One
    nasseg_augment_depth_colour launch (include/nasseg.h)."""
    return _augment("augment_depth_colour", src, desc, taps, lut, Ho, Wo, colour=(colour, ctab),
                    depth=(params, depth_scale))


def argmax_confusion(logits, gt, n_classes, cm=None, out_size=None, return_preds=False):
    """Fused bilinear up-sampling -> argmax -> uint8 -> confusion-matrix update.

    logits (B,C,h,w) fp32 on device, gt (B,H,W) uint8 on device; ``cm`` is an
    int64 (n,n) device tensor that is accumulated into (created when None).
    """
    logits = _cl(logits.detach())
    if logits.dtype != torch.float32:
        logits = logits.float()  # the reward path interpolates and compares in fp32
    B, C, h, w = logits.shape
    preds = None
    if gt is not None:
        require_device(gt)
        if gt.dtype != torch.uint8:
            raise NassegError("gt must be uint8")
        gt = gt.contiguous()
        H, W = gt.shape[1], gt.shape[2]
        if cm is None:
            cm = torch.zeros((n_classes, n_classes), device=logits.device, dtype=torch.int64)
    else:
        H, W = (int(out_size[0]), int(out_size[1])) if out_size is not None else (h, w)
    if return_preds:
        preds = torch.empty((B, H, W), device=logits.device, dtype=torch.uint8)
    lib.call("nasseg_argmax_cm", ptr(logits), ptr(gt), ptr(preds), B, h, w, C, H, W,
             int(n_classes), ptr(cm) if gt is not None else None, current_stream())
    return (cm, preds) if return_preds else cm


# ---------------------------------------------------------------------------
# prediction: image preparation and the notebooks' post-processing (engine/predict.py)
# ---------------------------------------------------------------------------
_TABLES_KEPT = 256  # device tables of each kind kept for reuse (least recently used first out)
_CUBIC_TABLES = collections.OrderedDict()
_PREPARE_PLANS = collections.OrderedDict()


def _lru(cache, key, make):
    hit = cache.get(key)
    if hit is None:
        hit = cache[key] = make()
        while len(cache) > _TABLES_KEPT:
            cache.popitem(last=False)
    else:
        cache.move_to_end(key)
    return hit


def cubic_tables_host(h, w, H, W):
    """(taps int32 [4 (H + W)], coef float32 [4 (H + W)]) of an h x w -> H x W INTER_CUBIC resize in cv2's dsize
    form: data/datasets._cubic_taps per axis, rows then columns (include/nasseg.h: nasseg_resize_cubic)."""
    import numpy as np

    from .data.datasets import _cubic_taps

    iy, wy = _cubic_taps(h, H, H / h)
    ix, wx = _cubic_taps(w, W, W / w)
    return (np.concatenate([iy.ravel(), ix.ravel()]).astype(np.int32),
            np.concatenate([wy.ravel(), wx.ravel()]).astype(np.float32))


def cubic_tables(device, h, w, H, W):
    """``cubic_tables_host`` uploaded to ``device``, cached per (device, h, w, H, W).  A caller that records the
    resize into a hipGraph holds on to the pair it passes (``tables=``): the cache may drop it later."""
    def make():
        taps, coef = cubic_tables_host(h, w, H, W)
        return torch.from_numpy(taps).to(device), torch.from_numpy(coef).to(device)

    return _lru(_CUBIC_TABLES, (torch.device(device), int(h), int(w), int(H), int(W)), make)


def _resize_args(name, x, size, tables):
    x = _cl(x.detach())
    B, C, h, w = x.shape
    try:
        H, W = (int(s) for s in size)
        ok = H > 0 and W > 0 and (H, W) == tuple(size)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise NassegError("{}: size must be two positive integers (got {!r})".format(name, size))
    if min(B, C, h, w) == 0:
        raise NassegError("{}: empty input {}".format(name, tuple(x.shape)))
    taps, coef = tables if tables is not None else cubic_tables(x.device, h, w, H, W)
    if (taps.dtype != torch.int32 or coef.dtype != torch.float32 or taps.numel() != 4 * (H + W)
            or coef.numel() != 4 * (H + W) or taps.device != x.device or coef.device != x.device):
        raise NassegError("{}: tables do not match a resize to {}x{}".format(name, H, W))
    return x, B, C, h, w, H, W, taps, coef


def resize_cubic(x, size, tables=None):
    """cv2.resize(logits, (W, H), interpolation=INTER_CUBIC) per channel: x B x C x h x w (channels_last, fp32 or
    bf16) -> fp32 B x C x H x W channels_last, bit-identical to data/datasets.resize_cubic_to; one
    nasseg_resize_cubic launch.  ``tables``: the pair ``cubic_tables`` returns for this resize."""
    x, B, C, h, w, H, W, taps, coef = _resize_args("resize_cubic", x, size, tables)
    y = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32, memory_format=torch.channels_last)
    lib.call(_k("nasseg_resize_cubic", x), ptr(x), B, h, w, C, ptr(taps), ptr(coef), ptr(y), H, W, current_stream())
    return y


def resize_cubic_argmax(x, size, tables=None):
    """argmax over C of ``resize_cubic(x, size)`` -> uint8 B x H x W (lowest index wins ties), the resized values
    never stored; at most 256 channels.  One nasseg_resize_cubic_argmax launch."""
    x, B, C, h, w, H, W, taps, coef = _resize_args("resize_cubic_argmax", x, size, tables)
    if C > 256:
        raise NassegError("resize_cubic_argmax: {} channels do not fit uint8 labels".format(C))
    labels = torch.empty((B, H, W), device=x.device, dtype=torch.uint8)
    lib.call(_k("nasseg_resize_cubic_argmax", x), ptr(x), B, h, w, C, ptr(taps), ptr(coef), ptr(labels), H, W,
             current_stream())
    return labels


# -- test-time ensemble over scales and mirroring (csrc/ensemble.hip) ---------------------------------------------
MAX_VIEWS = 16         # views one nasseg_fuse_views launch fuses
MAX_FUSE_CLASSES = 64  # channels of a fused view (the kernel's per-pixel sums live in registers)
FUSE_MODES = {"cubic": 4, "bilinear": 2}  # taps per axis
_FUSE_TABLES = collections.OrderedDict()


def view_size(n, s):
    """the side of a view's network input for an image side n at scale s: max(1, floor(n s + 0.5))"""
    import math

    return max(1, int(math.floor(n * s + 0.5)))


def _size_pair(name, size):
    try:
        H, W = (int(s) for s in size)
        ok = H > 0 and W > 0 and (H, W) == tuple(size)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise NassegError("{}: size must be two positive integers (got {!r})".format(name, size))
    return H, W


def view_image(x, size, mirror=False):
    """The network input of one view: x B x C x Hi x Wi (channels_last, fp32 or bf16) resized bilinearly to ``size``
    with align_corners=False (torch's F.interpolate, nasseg_bilinear_fwd's arithmetic) and, ``mirror``, with its
    columns reversed; one nasseg_view_image launch."""
    x = _cl(x.detach())
    B, C, Hi, Wi = x.shape
    Ho, Wo = _size_pair("view_image", size)
    if min(B, C, Hi, Wi) == 0:
        raise NassegError("view_image: empty input {}".format(tuple(x.shape)))
    y = _new(x, B, C, Ho, Wo)
    lib.call(_k("nasseg_view_image", x), ptr(x), ptr(y), B, Hi, Wi, C, Ho, Wo, int(bool(mirror)), current_stream())
    return y


def linear_tables_host(h, w, H, W):
    """(taps int32 [2 (H + W)], coef float32 [2 (H + W)]) of an h x w -> H x W bilinear resize with
    align_corners=False, rows then columns: torch's area_pixel_compute_source_index in fp32 (csrc/resize_index.h) -
    scale = in / out, src = max(scale (dst + 0.5) - 0.5, 0), taps floor(src) and the next (clipped), weights
    1 - frac and frac; equal sizes: the identity."""
    import numpy as np

    out = []
    for n_src, n_dst in ((h, H), (w, W)):
        d = np.arange(n_dst, dtype=np.float32)
        if n_src == n_dst:
            src = d
        else:
            scale = np.float32(n_src) / np.float32(n_dst)
            src = np.maximum(scale * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0))
        i0 = np.minimum(src.astype(np.int64), n_src - 1)
        i1 = np.minimum(i0 + 1, n_src - 1)
        l1 = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
        out.append((np.stack([i0, i1], 1), np.stack([np.float32(1) - l1, l1], 1)))
    (iy, wy), (ix, wx) = out
    return (np.concatenate([iy.ravel(), ix.ravel()]).astype(np.int32),
            np.concatenate([wy.ravel(), wx.ravel()]).astype(np.float32))


def fuse_tables_host(shapes, mirrored, H, W, mode="cubic"):
    """The tables of ``fuse_views``: per view (h, w) of ``shapes`` a block of T (H + W) entries, T = 4
    (``cubic_tables_host``) or 2 (``linear_tables_host``).  A mirrored view is un-mirrored here: its column taps t
    become w - 1 - t (the weights and the order of the taps stay: the sums are those of the resize of the flipped
    map).  Returns (taps int32, coef float32, dims int32 [V][3] = h, w, offset of the block)."""
    import numpy as np

    if mode not in FUSE_MODES:
        raise NassegError("fuse_views: mode must be one of {} (got {!r})".format(sorted(FUSE_MODES), mode))
    T = FUSE_MODES[mode]
    shapes = [(int(h), int(w)) for h, w in shapes]
    mirrored = [bool(m) for m in mirrored]
    if not shapes or len(shapes) != len(mirrored):
        raise NassegError("fuse_views: {} shapes and {} mirror flags".format(len(shapes), len(mirrored)))
    taps, coef, dims = [], [], []
    for (h, w), m in zip(shapes, mirrored):
        t, c = (cubic_tables_host if T == 4 else linear_tables_host)(h, w, H, W)
        if m:
            t = t.copy()
            t[T * H:] = w - 1 - t[T * H:]
        dims.append((h, w, len(taps) * T * (H + W)))
        taps.append(t)
        coef.append(c)
    return np.concatenate(taps), np.concatenate(coef), np.asarray(dims, np.int32)


def fuse_tables(device, shapes, mirrored, H, W, mode="cubic"):
    """``fuse_tables_host`` with taps and coef uploaded to ``device`` (dims stays on the host), cached per argument
    list.  A caller that records the fusion into a hipGraph holds on to what it passes (``tables=``): the cache may
    drop it later."""
    shapes = tuple((int(h), int(w)) for h, w in shapes)
    mirrored = tuple(bool(m) for m in mirrored)

    def make():
        taps, coef, dims = fuse_tables_host(shapes, mirrored, H, W, mode)
        return torch.from_numpy(taps).to(device), torch.from_numpy(coef).to(device), dims

    return _lru(_FUSE_TABLES, (torch.device(device), shapes, mirrored, int(H), int(W), mode), make)


def _fuse(name, views, size, mirrored, mode, tables, gt, n_classes, cm, want_labels, want_probs, want_mean):
    views = [_cl(v.detach()) for v in views]
    if not views or len(views) > MAX_VIEWS:
        raise NassegError("{}: between 1 and {} views (got {})".format(name, MAX_VIEWS, len(views)))
    B, C = views[0].shape[:2]
    first = views[0]
    for v in views:
        if v.dtype != first.dtype or v.device != first.device or tuple(v.shape[:2]) != (B, C) or v.numel() == 0:
            raise NassegError("{}: the views differ in dtype, device, batch or channels, or one is empty".format(name))
    if C > MAX_FUSE_CLASSES:
        raise NassegError("{}: {} channels (at most {})".format(name, C, MAX_FUSE_CLASSES))
    H, W = _size_pair(name, size)
    mirrored = [bool(m) for m in mirrored]
    if len(mirrored) != len(views):
        raise NassegError("{}: {} views and {} mirror flags".format(name, len(views), len(mirrored)))
    if mode not in FUSE_MODES:
        raise NassegError("{}: mode must be one of {} (got {!r})".format(name, sorted(FUSE_MODES), mode))
    T = FUSE_MODES[mode]
    shapes = [tuple(v.shape[2:]) for v in views]
    taps, coef, dims = tables if tables is not None else fuse_tables(first.device, shapes, mirrored, H, W, mode)
    n = len(views) * T * (H + W)
    if (taps.dtype != torch.int32 or coef.dtype != torch.float32 or taps.numel() != n or coef.numel() != n
            or taps.device != first.device or coef.device != first.device or tuple(dims.shape) != (len(views), 3)
            or [tuple(d[:2]) for d in dims.tolist()] != [tuple(s) for s in shapes]
            or any(d[2] < 0 or d[2] + T * (H + W) > n for d in dims.tolist())):
        raise NassegError("{}: tables do not match {} views resized to {}x{}".format(name, len(views), H, W))
    if gt is not None:
        require_device(gt)
        if gt.dtype != torch.uint8 or tuple(gt.shape) != (B, H, W):
            raise NassegError("{}: gt must be uint8 {} (got {} {})".format(name, (B, H, W), gt.dtype, tuple(gt.shape)))
        gt = gt.contiguous()
        if n_classes is None:
            raise NassegError("{}: gt needs n_classes".format(name))
        n_classes = int(n_classes)
        if not 0 < n_classes <= 256:
            raise NassegError("{}: n_classes={} (at most 256)".format(name, n_classes))
        if cm is None:
            cm = torch.zeros((n_classes, n_classes), device=first.device, dtype=torch.int64)
        elif (cm.dtype != torch.int64 or tuple(cm.shape) != (n_classes, n_classes) or not cm.is_contiguous()
              or cm.device != first.device):
            raise NassegError("{}: cm must be a contiguous int64 {} tensor on the device".format(
                name, (n_classes, n_classes)))
    else:
        cm = None
    dev = first.device
    labels = torch.empty((B, H, W), device=dev, dtype=torch.uint8) if want_labels else None
    probs = (torch.empty((B, C, H, W), device=dev, dtype=torch.float32, memory_format=torch.channels_last)
             if want_probs else None)
    mean = (torch.empty((B, C, H, W), device=dev, dtype=torch.float32, memory_format=torch.channels_last)
            if want_mean else None)
    table = (ctypes.c_void_p * len(views))(*[ptr(v) for v in views])
    hdims = (ctypes.c_int * (3 * len(views)))(*[int(d) for d in dims.ravel()])
    if lib.recorder is not None:  # (the pointer table: what the launch reads behind it)
        lib.recorder.annotate(reads=views + [taps, coef, gt], writes=[labels, probs, cm, mean])
    lib.call(_k("nasseg_fuse_views", first), len(views), table, hdims, ptr(taps), ptr(coef), T, B, C, H, W, ptr(gt),
             n_classes if cm is not None else 0, ptr(labels), ptr(probs), ptr(cm), ptr(mean), current_stream())
    return labels, probs, cm, mean


def fuse_views(views, size, mirrored, mode="cubic", gt=None, n_classes=None, cm=None, return_probs=False,
               tables=None, return_mean=False):
    """The ensemble of V <= 16 views in ONE nasseg_fuse_views launch: views[v] B x C x h_v x w_v logits (channels_last,
    all fp32 or all bf16, C <= 64), ``mirrored[v]``: the view's image was mirrored.  Every view is resampled to
    ``size`` (mode "cubic": ``resize_cubic``'s arithmetic bit for bit; "bilinear": align_corners=False), soft-maxed
    over C in fp32, the probabilities are added in view order and the label is their argmax (lowest index wins
    ties) - nothing of a view is stored at full resolution.

    Returns uint8 labels B x H x W; with ``gt`` (uint8 B x H x W) and ``n_classes``: (cm, labels), the int64
    confusion matrix ``cm`` (created when None) accumulated over the pixels with gt < n_classes as
    ``argmax_confusion`` does.  ``return_probs`` appends the mean probabilities, ``return_mean`` the mean of the
    resampled views (both fp32 B x C x H x W channels_last).  ``tables``: what ``fuse_tables`` returns for it."""
    labels, probs, cm, mean = _fuse("fuse_views", views, size, mirrored, mode, tables, gt, n_classes, cm, True,
                                    return_probs, return_mean)
    out = ([cm] if gt is not None else []) + [labels] + ([probs] if return_probs else []) + (
        [mean] if return_mean else [])
    return out[0] if len(out) == 1 else tuple(out)


def fuse_views_mean(views, size, mirrored, mode="cubic", tables=None):
    """The mean over the views of their maps resampled to ``size`` (no softmax: depth) -> fp32 B x C x H x W
    channels_last; one nasseg_fuse_views launch.  One un-mirrored view, mode "cubic": ``resize_cubic``."""
    return _fuse("fuse_views_mean", views, size, mirrored, mode, tables, None, None, None, False, False, True)[3]


def prepare_plan(device, B, H, W, dtype=torch.float32):
    """(desc, taps, lut) of ``prepare_image`` for B images of H x W on ``device``: nasseg_augment's descriptor and
    tables with an identity plan - one tap per row and column, coefficients (0, 2048, 0, 0), so the fixed-point
    resize gives every uint8 value back - and the table of the reference's prepare_img (data/device.py).  Cached
    per (device, B, H, W, dtype); a caller recording the launch into a hipGraph holds on to what it passes."""
    import numpy as np

    from .data import device as ddev

    if dtype not in (torch.float32, torch.bfloat16):
        raise NassegError("prepare_image: images are float32 or bfloat16 (got {})".format(dtype))

    def make():
        axes = []
        for n in (H, W):
            c = np.arange(n, dtype=np.int64)
            axes.append((np.concatenate([np.repeat(c[:, None], 4, axis=1),
                                         np.broadcast_to(ddev._IDENTITY_COEF, (n, 4))], 1), c))
        (ty, my), (tx, mx) = axes
        taps = np.concatenate([ty.ravel(), tx.ravel(), my, mx]).astype(np.int32)
        desc = np.zeros((B, ddev.DESC_FIELDS), np.int64)
        desc[:] = ddev.Desc(img_off=0, msk_off=0, h=H, w=W, img_ld=3 * W, msk_ld=W, img_fill=0, msk_fill=0)
        desc[:, ddev.Desc._fields.index("img_off")] = np.arange(B, dtype=np.int64) * (H * W * 3)
        lut = torch.from_numpy(ddev.prepare_img_table()).float().to(dtype)
        return (torch.from_numpy(desc).to(device), torch.from_numpy(np.tile(taps, (B, 1))).to(device),
                lut.to(device))

    return _lru(_PREPARE_PLANS, (torch.device(device), int(B), int(H), int(W), dtype), make)


def prepare_image(img, dtype=torch.float32, plan=None):
    """The reference's ``torch.tensor(prepare_img(img).transpose(2, 0, 1)[None]).float()`` on the device, bit for
    bit: uint8 B x H x W x 3 (device) -> B x 3 x H x W channels_last ``dtype`` (fp32, or bf16 = that tensor
    rounded), one nasseg_augment launch without a mask.  ``plan``: what ``prepare_plan`` returns for it."""
    require_device(img)
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3 or img.numel() == 0:
        raise NassegError("prepare_image: expected a uint8 B x H x W x 3 image (got {} {})".format(
            img.dtype, tuple(img.shape)))
    B, H, W, _ = img.shape
    img = img.contiguous()
    desc, taps, lut = plan if plan is not None else prepare_plan(img.device, B, H, W, dtype)
    if (lut.dtype != dtype or tuple(desc.shape) != (B, 8) or tuple(taps.shape) != (B, 9 * (H + W))
            or desc.device != img.device):
        raise NassegError("prepare_image: the plan does not match a {} batch of {}x{}".format(B, H, W))
    image = torch.empty((B, 3, H, W), device=img.device, dtype=dtype, memory_format=torch.channels_last)
    lib.call(_k("nasseg_augment", image), ptr(img), img.numel(), ptr(desc), ptr(taps), ptr(lut), ptr(image), None,
             B, H, W, current_stream())
    return image


# -- the search controller (csrc/controller.hip) ---------------------------------------------------------------------
class ControllerPlan(object):
    """What the controller kernels need to know about a controller, built once per module (rl/micro_controllers.py):
    ``steps`` = [(head index or -1, choices, position in an action row or -1)] per LSTM step, ``head_rows`` = choices
    per head.  Parameters are handed to the calls as a list in TABLE ORDER - g_emb, then weight_ih / weight_hh /
    bias_ih / bias_hh per LSTM layer, then weight and bias per head - and reach the kernels as a device table of their
    addresses: the table is rebuilt when an address changes, the values are never copied, so nothing goes stale after
    an optimiser step.  A hipGraph captured around these calls has the table's and the parameters' addresses baked in:
    it is valid as long as the parameters stay where they are (in-place updates, as optimisers make them), and has to
    be captured again after they were re-allocated (``.to()``,
    ``load_state_dict(assign=True)``).  Gradients come back as slices of one flat buffer laid out by ``offsets``."""

    def __init__(self, steps, hidden, layers, head_rows, action_len):
        self.steps = [tuple(int(v) for v in s) for s in steps]
        self.T, self.H, self.L, self.A = len(self.steps), int(hidden), int(layers), int(action_len)
        self.head_rows = [int(n) for n in head_rows]
        self.NH = len(self.head_rows)
        self.maxn = max(self.head_rows) if self.head_rows else 0
        H = self.H
        self.shapes = [(H,)] + [s for _ in range(self.L) for s in ((4 * H, H), (4 * H, H), (4 * H,), (4 * H,))]
        self.shapes += [s for n in self.head_rows for s in ((n, H), (n,))]
        self.numels = [int(np.prod(s)) for s in self.shapes]
        self.offsets, off = [], 0
        for n in self.numels:
            self.offsets.append(off)
            off += (n + 3) // 4 * 4  # (every slice 16-byte aligned)
        self.total = off
        self._static = {}  # device -> (steps, gtab)
        self._ptab = {}    # device -> (addresses, table)

    def tables(self, params):
        """(parameter addresses, step table, gradient table) on the parameters' device"""
        if len(params) != len(self.shapes):
            raise NassegError("controller: {} parameters for a table of {}".format(len(params), len(self.shapes)))
        require_device(*params)
        for p, shape in zip(params, self.shapes):
            if p.dtype != torch.float32 or p.numel() != int(np.prod(shape)) or not p.is_contiguous():
                raise NassegError("controller: parameters must be contiguous fp32 of {} elements (got {} {})".format(
                    int(np.prod(shape)), p.dtype, tuple(p.shape)))
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise NassegError("controller: parameters on several devices")
        static = self._static.get(dev)
        if static is None:
            rows = [1] + [4 * self.H] * (4 * self.L) + [n for n in self.head_rows for _ in (0, 1)]
            static = (torch.tensor(self.steps, dtype=torch.int32, device=dev).reshape(-1, 3).contiguous(),
                      torch.tensor(list(zip(self.offsets, rows)), dtype=torch.int32, device=dev).contiguous())
            self._static[dev] = static
        key = tuple(p.data_ptr() for p in params)
        ent = self._ptab.get(dev)
        if ent is None or ent[0] != key:
            ent = (key, torch.tensor(key, dtype=torch.int64, device=dev))
            self._ptab[dev] = ent
        return ent[1], static[0], static[1]

    def dims(self):
        return (self.T, self.H, self.L, self.NH, self.maxn)

    def split(self, flat):
        """the parameters' gradients: slices of the flat buffer, in table order"""
        return [flat[o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, self.shapes)]


def _ctrl_rows(plan, actions, rows):
    """(actions, rows, n_rows, B) as the kernels take them"""
    if actions is None:
        return None, None, 0, 0
    if actions.dtype != torch.int32 or actions.dim() != 2 or actions.shape[1] != plan.A or not actions.is_contiguous():
        raise NassegError("controller: actions must be a contiguous int32 (rows, {}) tensor (got {} {})".format(
            plan.A, actions.dtype, tuple(actions.shape)))
    require_device(actions, rows)
    if rows is not None and (rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous()):
        raise NassegError("controller: rows must be a contiguous int32 vector")
    n_rows = int(actions.shape[0])
    return actions, rows, n_rows, (n_rows if rows is None else int(rows.shape[0]))


def controller_forward(plan, params, actions=None, rows=None, u=None):
    """One nasseg_ctrl_rollout launch, no autograd: -> (entropy (), log_prob (B,), saved, sampled (n, A) int32 or None,
    sampled log_prob (n,) or None).  ``saved`` is what ``controller_backward`` reads."""
    ptab, steps, _ = plan.tables(params)
    actions, rows, n_rows, B = _ctrl_rows(plan, actions, rows)
    like = params[0]
    T, H, L, NH, maxn = plan.dims()
    n, sampled, sampled_lp = 0, None, None
    if u is not None:
        require_device(u)
        if u.dtype != torch.float32 or u.dim() != 2 or u.shape[1] != T or not u.is_contiguous():
            raise NassegError("controller: uniforms must be a contiguous fp32 (n, {}) tensor".format(T))
        n = int(u.shape[0])
        sampled = torch.empty((n, plan.A), device=like.device, dtype=torch.int32)
        sampled_lp = torch.empty((n,), device=like.device, dtype=torch.float32)
    saved = _ws(like, lib.query("nasseg_ctrl_saved_floats", T, H, L))
    entropy = _scalar(like)
    log_prob = torch.empty((B,), device=like.device, dtype=torch.float32)
    lib.call("nasseg_ctrl_rollout", ptr(ptab), ptr(steps), T, H, L, NH, maxn, ptr(actions), ptr(rows), n_rows, B,
             plan.A, ptr(u), n, ptr(sampled), ptr(sampled_lp), ptr(saved), ptr(entropy),
             ptr(log_prob) if B else None, current_stream())
    return entropy, log_prob, saved, sampled, sampled_lp


def controller_backward(plan, params, saved, actions, rows, d_log_prob, d_entropy, flat=None, work=None):
    """The two nasseg_ctrl_backward launches (the chain in one workgroup, then the parameter gradients), no autograd:
    writes every parameter's gradient into ``flat`` (plan.total floats, made when None) and returns it."""
    ptab, steps, gtab = plan.tables(params)
    actions, rows, n_rows, B = _ctrl_rows(plan, actions, rows)
    T, H, L, NH, maxn = plan.dims()
    if flat is None:
        flat = _ws(params[0], plan.total)
    if work is None:
        work = _ws(params[0], lib.query("nasseg_ctrl_work_floats", T, H, L))
    lib.call("nasseg_ctrl_backward", ptr(ptab), ptr(steps), T, H, L, NH, maxn, ptr(actions), ptr(rows), n_rows, B,
             plan.A, ptr(d_log_prob) if B else None, ptr(d_entropy), ptr(saved), ptr(work), ptr(gtab), ptr(flat),
             current_stream())
    return flat


class _ControllerRollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, actions, rows, *params):
        entropy, log_prob, saved, _, _ = controller_forward(plan, params, actions, rows)
        ctx.plan = plan
        ctx.save_for_backward(saved, actions, rows, *params)
        return entropy, log_prob

    @staticmethod
    def backward(ctx, g_ent, g_lp):
        saved, actions, rows = ctx.saved_tensors[:3]
        params = ctx.saved_tensors[3:]
        plan = ctx.plan
        if g_ent is not None:
            g_ent = g_ent.to(torch.float32).contiguous()
        if g_lp is not None:
            g_lp = g_lp.to(torch.float32).contiguous()
        flat = controller_backward(plan, params, saved, actions if g_lp is not None else None,
                                   rows if g_lp is not None else None, g_lp, g_ent)
        grads = plan.split(flat)
        return (None, None, None) + tuple(g.view_as(p) if need else None
                                           for g, p, need in zip(grads, params, ctx.needs_input_grad[3:]))


def controller_rollout(plan, params, actions=None, rows=None):
    """The controller's T-step rollout as ONE autograd node: -> (entropy, log_probs) - the total entropy of the
    steps' distributions (0-dim) and, for the B action rows ``actions[rows]`` (int32 (n_rows, A); rows None: all of
    them; actions None: B = 0), log_probs (B,).  Backward: the two nasseg_ctrl_backward launches.  Both results are
    tensors of their own (``loss += ...`` on them works)."""
    return _ControllerRollout.apply(plan, actions, rows, *params)


def controller_sample(plan, params, u):
    """Sample u.shape[0] candidates from ONE rollout by inverse CDF of the uniforms u (n, T): -> (actions int32 (n, A),
    log_probs (n,), entropy ()); no autograd."""
    with torch.no_grad():
        entropy, _, _, sampled, sampled_lp = controller_forward(plan, [p.detach() for p in params], u=u)
    return sampled, sampled_lp, entropy


def controller_ppo_seed(log_prob, entropy, old_log_prob, adv, rows, clip_param, entropy_coef, acc, d_log_prob,
                        d_entropy):
    """The PPO surrogate on the device (nasseg_ctrl_ppo_seed): adds action_loss and entropy to ``acc`` (2,) and
    writes the gradients of action_loss - entropy_coef * entropy into d_log_prob (B,) and d_entropy ()."""
    require_device(log_prob, entropy, old_log_prob, adv, rows, acc, d_log_prob, d_entropy)
    lib.call("nasseg_ctrl_ppo_seed", ptr(log_prob), ptr(entropy), ptr(old_log_prob), ptr(adv), ptr(rows),
             int(old_log_prob.numel()), int(log_prob.numel()), float(1.0 - clip_param), float(1.0 + clip_param),
             float(entropy_coef), ptr(acc), ptr(d_log_prob), ptr(d_entropy), current_stream())


def _apply_library_knobs():
    if _PW_MIN_PIXELS is not None:
        lib.query("nasseg_conv_pw_min_pixels", int(_PW_MIN_PIXELS))
        lib._memo.clear()
    if _PWN_MODE is not None:
        lib.query("nasseg_conv_pwn_mode", int(_PWN_MODE))
        lib._memo.clear()
    # NASSEG_DW_WGRAD_LDS=0: the strip kernel for 5x5 depthwise weight gradients too; NASSEG_CONV_DEEP_K=0: one
    # k-step per round trip on small maps as well; NASSEG_POOL_STRIP=0 / 2: stride-1 max pooling one gather per
    # element / two rows per thread; NASSEG_PW_RZ_MIN_PIXELS: maps from which the one-kernel pointwise backward rebuilds
    # z instead of loading it (A/B switches, include/nasseg.h)
    for env, fn in (("NASSEG_DW_WGRAD_LDS", "nasseg_dw_wgrad_lds"), ("NASSEG_CONV_DEEP_K", "nasseg_conv_deep_k"),
                    ("NASSEG_POOL_STRIP", "nasseg_pool_strip"),
                    ("NASSEG_PW_RZ_MIN_PIXELS", "nasseg_conv_pw_bwd_rz_min_pixels")):
        if os.environ.get(env) is not None:
            lib.query(fn, int(os.environ[env]))
            lib._memo.clear()


try:
    _apply_library_knobs()
except (OSError, NassegError):  # (no library yet - a CPU-only import before the build; set again after loading)
    pass
