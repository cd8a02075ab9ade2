"""Host-side owner of the native handle: turns a graph IR + state_dict into a planned backbone
inside `libi2v_hip.so` and exposes forward-to-hooks / backward-to-input on torch tensors.

PyTorch is used for device memory and streams only (`tensor.data_ptr()`,
`torch.cuda.current_stream().cuda_stream`); all arithmetic happens behind the C ABI.
"""
import ctypes as C
import sys
import threading
import time
from typing import List, Sequence

import torch

from . import lib as _lib
from .graphs import FAMILIES, FAMILY_OF, Graph
from .weights import fold_affine, fold_pre_affine


_DEVICE_TYPES = {}          # device type -> number of engines ALIVE on it in this process ('cuda' for libi2v_hip.so)


def _ptr(t: torch.Tensor, eng: "Engine" = None):
    """Device pointer of a tensor handed to the library.  With `eng` the tensor must live on that engine's device type (every
    call that knows its engine passes it); without, on the device type of some engine that is still alive (an entry goes
    when its last engine closes -- a host-simulation engine that once existed does not let CPU tensors through for good)."""
    assert t.is_contiguous() and t.dtype == torch.float32, (t.dtype, t.is_contiguous())
    ok = t.device.type == eng.device.type if eng is not None else _DEVICE_TYPES.get(t.device.type, 0) > 0
    if not ok:      # a host pointer handed to a HIP kernel reads garbage or faults the GPU
        where = eng.device if eng is not None else sorted(k for k, v in _DEVICE_TYPES.items() if v > 0)
        raise _lib.I2VError(f"tensor on {t.device} passed to an engine on {where}: move it to the engine's device")
    return C.c_void_p(t.data_ptr())


def _hptr(t: torch.Tensor):
    """HOST array handed to the description calls (`i2v_net_add_conv*` take host weights / scale / shift)."""
    assert t.is_contiguous() and t.dtype == torch.float32 and t.device.type == "cpu", (t.dtype, t.device)
    return C.c_void_p(t.data_ptr())


class Engine:
    """One per (process, device) -- mirrors the reference's single `.cuda()` device
    (`image_attacks.py:103`).  `capi` is injected only by the planner unit tests.  The `build_<word>_net` methods of the transformer
    families are set in the loop directly behind this class."""

    def __init__(self, device="cuda:0", capi=None):
        self.device = torch.device(device)
        self.capi = capi if capi is not None else _lib.load()
        if capi is None and self.device.type != "cuda":
            raise _lib.I2VError("the I2V engine needs a ROCm device; there is no CPU path")
        self.h = C.c_void_p()
        # net creation / planning / destruction touch the handle's net table.  Re-entrant: Net.__del__ -> close() takes it, and the
        # cyclic GC may finalise an unreachable Net on the very thread that is inside build_net
        self.plan_lock = threading.RLock()
        self.plan_ms, self.plans = 0.0, 0      # host wall time spent building nets (never inside a timed region of bench.py)
        idx = self.device.index or 0
        _lib.check(self.capi, self.capi.i2v_create(idx, C.byref(self.h)))
        _DEVICE_TYPES[self.device.type] = _DEVICE_TYPES.get(self.device.type, 0) + 1

    def stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def close(self):
        if self.h:
            self.capi.i2v_destroy(self.h)
            self.h = C.c_void_p()
            _DEVICE_TYPES[self.device.type] = max(0, _DEVICE_TYPES.get(self.device.type, 0) - 1)

    def __del__(self):
        try:
            if not sys.is_finalizing():        # at interpreter exit the HIP runtime may already be tearing down: let the OS reclaim
                self.close()
        except Exception:
            pass

    def _build(self, cls, *args):
        """Thread-safe (concurrent clip streams plan their own nets); execution of DIFFERENT nets on different
        streams needs no lock -- a planned net owns its arena, the library keeps no other mutable state."""
        with self.plan_lock:
            t0 = time.perf_counter()
            net = cls(self, *args)
            self.plan_ms += 1e3 * (time.perf_counter() - t0)      # pack + upload + plan + autotune (i2v_net_plan syncs)
            self.plans += 1
            return net

    def build_net(self, graph: Graph, state_dict, hook_tensors: Sequence[int], max_frames: int, relu_gain=None) -> "Net":
        return self._build(Net, graph, state_dict, list(hook_tensors), max_frames, relu_gain)

    def build_token_net(self, spec, state_dict, hooks: Sequence[int], max_frames: int) -> "TokenNet":
        """A transformer surrogate of whichever family `spec` belongs to (`graphs.FAMILIES`; `include/i2v_<word>.h`): weights packed
        and uploaded and the arena planned for up to `max_frames` frames.  The `build_<word>_net` methods are this call."""
        return self._build(TokenNet, spec, state_dict, list(hooks), max_frames)

    def convnext_dw(self, x: torch.Tensor, filt: torch.Tensor, bias=None, add=None) -> torch.Tensor:
        """The ConvNeXt block's depthwise 7 x 7 launch on its own (`i2v_convnext_dw_f32`): x (frames, H, W, C) token-major, filt (49, C),
        optional bias (C) and addend (frames, H, W, C) -> (frames, H, W, C)."""
        n, H, W, Cn = x.shape
        assert tuple(filt.shape) == (49, Cn)
        y = torch.empty_like(x)
        _lib.check(self.capi, self.capi.i2v_convnext_dw_f32(_ptr(x, self), _ptr(filt, self), _ptr(bias, self) if bias is not None else None,
                                                            _ptr(add, self) if add is not None else None, _ptr(y, self), n, H, W, Cn,
                                                            self.stream()))
        return y

    def mixer_tokens(self, z: torch.Tensor, residual: torch.Tensor, w1, b1, w2=None, b2=None, in_scale=None, in_shift=None, out_scale=None,
                     channel_tile: int = 0) -> torch.Tensor:
        """The token-mixing launch on its own (`i2v_mixer_tokens_f32`): z, residual (frames, S, C) token-major; w1 (Sh, S), b1 (Sh),
        w2 (S, Sh), b2 (S) -- or, without w2, the one Linear w1 (S, S), b1 (S) of ResMLP; optional per-channel in_scale / in_shift /
        out_scale -> residual + out_scale * tokmix(in_scale * z + in_shift), (frames, S, C)."""
        n, S, Cn = z.shape
        Sh = 0 if w2 is None else w1.shape[0]
        assert tuple(w1.shape) == ((Sh, S) if Sh else (S, S)) and (w2 is None or tuple(w2.shape) == (S, Sh))
        out = torch.empty_like(z)
        o = lambda t: _ptr(t, self) if t is not None else None      # noqa: E731
        _lib.check(self.capi, self.capi.i2v_mixer_tokens_f32(_ptr(z, self), _ptr(residual, self), _ptr(out, self), n, S, Sh, Cn, _ptr(w1, self),
                                                             _ptr(b1, self), o(w2), o(b2), o(in_scale), o(in_shift), o(out_scale),
                                                             channel_tile, self.stream()))
        return out

    def mixer_tokens_bwd(self, z, g: torch.Tensor, w1, b1, w2=None, in_scale=None, in_shift=None, out_scale=None, add=None,
                         channel_tile: int = 0) -> torch.Tensor:
        """The input gradient of that launch (`i2v_mixer_tokens_bwd_f32`) from g = d(out), plus `add`: the transposed copies the entry
        wants are made here.  Without w2 (ResMLP) z and b1 are not needed."""
        n, S, Cn = g.shape
        Sh = 0 if w2 is None else w1.shape[0]
        w2t = (w2 if Sh else w1).t().contiguous()
        w1t = w1.t().contiguous() if Sh else None
        dz = torch.empty_like(g)
        o = lambda t: _ptr(t, self) if t is not None else None      # noqa: E731
        _lib.check(self.capi, self.capi.i2v_mixer_tokens_bwd_f32(o(z if Sh else None), _ptr(g, self), o(add), _ptr(dz, self), n, S, Sh, Cn,
                                                                 o(w1 if Sh else None), o(b1 if Sh else None), _ptr(w2t, self), o(w1t),
                                                                 o(in_scale), o(in_shift), o(out_scale), channel_tile, self.stream()))
        return dz

    def cait_attention(self, qkv: torch.Tensor, heads: int, scale: float, wl, bl, ww, bw):
        """Talking-heads attention on its own (`i2v_cait_attention_f32`): qkv (frames, T, 3 heads dh) as the ViT entry takes it, wl / ww
        (heads, heads), bl / bw (heads) -> (out (frames, T, heads dh), probs (frames, heads, T, ld): post-softmax, pre-mix)."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        assert 3 * heads * dh == C3 and tuple(wl.shape) == tuple(ww.shape) == (heads, heads)
        ld = (T + 3) // 4 * 4
        probs = torch.zeros(n, heads, T, ld, dtype=torch.float32, device=qkv.device)
        out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
        _lib.check(self.capi, self.capi.i2v_cait_attention_f32(_ptr(qkv, self), n, T, heads, dh, scale, _ptr(wl, self), _ptr(bl, self),
                                                               _ptr(ww, self), _ptr(bw, self), _ptr(probs, self), _ptr(out, self), self.stream()))
        return out, probs

    def cait_attention_bwd(self, qkv: torch.Tensor, probs: torch.Tensor, dout: torch.Tensor, heads: int, scale: float, wl, ww, bw) -> torch.Tensor:
        """The input gradient of that launch (`i2v_cait_attention_bwd_f32`) from dout = d(out): dqkv (frames, T, 3 heads dh).  The two
        scratch arrays of the probabilities' size are made here."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        ds, pm = torch.empty_like(probs), torch.empty_like(probs)
        dqkv = torch.empty_like(qkv)
        _lib.check(self.capi, self.capi.i2v_cait_attention_bwd_f32(_ptr(qkv, self), _ptr(probs, self), _ptr(dout, self), n, T, heads, dh, scale,
                                                                   _ptr(wl, self), _ptr(ww, self), _ptr(bw, self), _ptr(ds, self), _ptr(pm, self),
                                                                   _ptr(dqkv, self), self.stream()))
        return dqkv

    def convit_attention(self, qkv: torch.Tensor, heads: int, scale: float, c=None, table=None):
        """Gated positional attention on its own (`i2v_convit_attention_f32`): qkv (frames, T, 3 heads dh) as the ViT entry takes it, c
        (heads), table (heads, T, ld) non-negative with ld = T rounded up to 4; both None: plain attention -> (out (frames, T, heads dh)
        = fma(c, Ppatch, table) v, probs (frames, heads, T, ld): Ppatch, the softmax before the blend)."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        ld = (T + 3) // 4 * 4
        assert 3 * heads * dh == C3 and (table is None or tuple(table.shape) == (heads, T, ld))
        probs = torch.zeros(n, heads, T, ld, dtype=torch.float32, device=qkv.device)
        out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
        o = lambda t: None if t is None else _ptr(t, self)      # noqa: E731
        _lib.check(self.capi, self.capi.i2v_convit_attention_f32(_ptr(qkv, self), n, T, heads, dh, scale, o(c), o(table), _ptr(probs, self),
                                                                 _ptr(out, self), self.stream()))
        return out, probs

    def convit_attention_bwd(self, qkv: torch.Tensor, probs: torch.Tensor, dout: torch.Tensor, heads: int, scale: float, c=None,
                             table=None) -> torch.Tensor:
        """The input gradient of that launch (`i2v_convit_attention_bwd_f32`) from dout = d(out): dqkv (frames, T, 3 heads dh).  The
        scratch array of the probabilities' size is made here."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        ds = torch.empty_like(probs)
        dqkv = torch.empty_like(qkv)
        o = lambda t: None if t is None else _ptr(t, self)      # noqa: E731
        _lib.check(self.capi, self.capi.i2v_convit_attention_bwd_f32(_ptr(qkv, self), _ptr(probs, self), _ptr(dout, self), n, T, heads, dh, scale,
                                                                     o(c), o(table), _ptr(ds, self), _ptr(dqkv, self), self.stream()))
        return dqkv

    def xcit_attention(self, qkv: torch.Tensor, heads: int, temperature: torch.Tensor):
        """Cross-covariance attention on its own (`i2v_xcit_attention_f32`): qkv (frames, T, 3 heads dh) as the ViT entry takes it,
        temperature (heads) -> (out (frames, T, heads dh), probs (frames, heads, dh, dh), gram (frames, heads, dh + 2, dh): the normalised
        Gram, then the clamped column norms of q and of k)."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        assert 3 * heads * dh == C3
        gram = torch.zeros(n, heads, dh + 2, dh, dtype=torch.float32, device=qkv.device)
        probs = torch.zeros(n, heads, dh, dh, dtype=torch.float32, device=qkv.device)
        out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
        _lib.check(self.capi, self.capi.i2v_xcit_attention_f32(_ptr(qkv, self), n, T, heads, dh, _ptr(temperature, self), _ptr(gram, self),
                                                               _ptr(probs, self), _ptr(out, self), self.stream()))
        return out, probs, gram

    def xcit_attention_bwd(self, qkv: torch.Tensor, gram: torch.Tensor, probs: torch.Tensor, dout: torch.Tensor, heads: int,
                           temperature: torch.Tensor) -> torch.Tensor:
        """The input gradient of that launch (`i2v_xcit_attention_bwd_f32`) from dout = d(out): dqkv (frames, T, 3 heads dh)."""
        n, T, C3 = qkv.shape
        dqkv = torch.empty_like(qkv)
        _lib.check(self.capi, self.capi.i2v_xcit_attention_bwd_f32(_ptr(qkv, self), _ptr(gram, self), _ptr(probs, self), _ptr(dout, self), n, T,
                                                                   heads, C3 // (3 * heads), _ptr(temperature, self), _ptr(dqkv, self),
                                                                   self.stream()))
        return dqkv

    def xcit_dw3(self, x: torch.Tensor, w: torch.Tensor, bias=None, ta=None, ts=None, add=None, ma=None, mu=None) -> torch.Tensor:
        """The token-major depthwise 3 x 3 launch on its own (`i2v_xcit_dw3_f32`): x (n, H, W, C), w (9, C); the optional input transform
        ta * gelu(x) + ts, residual `add` and output multiply ma * gelu'(mu)."""
        n, H, W, Cn = x.shape
        y = torch.empty_like(x)
        o = lambda t: None if t is None else _ptr(t, self)      # noqa: E731
        _lib.check(self.capi, self.capi.i2v_xcit_dw3_f32(_ptr(x, self), n, H, W, Cn, _ptr(w, self), o(bias), o(ta), o(ts), o(add), o(ma), o(mu),
                                                         _ptr(y, self), self.stream()))
        return y

    def xcit_stem_gather(self, src: torch.Tensor, nchw: bool = False) -> torch.Tensor:
        """The stem's 3 x 3 / 2 / pad 1 gather on its own (`i2v_xcit_stem_gather_f32`): src (n, H, W, C), or (n, C, H, W) with `nchw` ->
        rows (n Ho Wo, 9 C)."""
        n, H, W, Cn = (src.shape[0], src.shape[2], src.shape[3], src.shape[1]) if nchw else src.shape
        rows = torch.empty(n * ((H + 1) // 2) * ((W + 1) // 2), 9 * Cn, dtype=torch.float32, device=src.device)
        _lib.check(self.capi, self.capi.i2v_xcit_stem_gather_f32(_ptr(src, self), _ptr(rows, self), n, H, W, Cn, int(nchw), self.stream()))
        return rows

    def xcit_stem_scatter(self, drows: torch.Tensor, shape, pre=None, nchw: bool = False, into=None) -> torch.Tensor:
        """Its transpose (`i2v_xcit_stem_scatter_f32`): drows (n Ho Wo, 9 C) -> the gradient of a source of `shape`, times gelu'(pre) where
        pre is given; `into` (image layout only) is added to."""
        n, H, W, Cn = (shape[0], shape[2], shape[3], shape[1]) if nchw else shape
        dst = into if into is not None else torch.empty(*shape, dtype=torch.float32, device=drows.device)
        _lib.check(self.capi, self.capi.i2v_xcit_stem_scatter_f32(_ptr(drows, self), None if pre is None else _ptr(pre, self), _ptr(dst, self),
                                                                  n, H, W, Cn, int(nchw), int(into is not None), self.stream()))
        return dst

    def twins_attention(self, q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float = None) -> torch.Tensor:
        """Sub-sampled attention on its own (`i2v_twins_attention_f32`): q (frames, Tq, heads dh), kv (frames, Tk, 2 heads dh) ->
        out (frames, Tq, heads dh); `scale` defaults to dh^-0.5."""
        n, Tq, Cn = q.shape
        dh = Cn // heads
        assert heads * dh == Cn and kv.shape[0] == n and kv.shape[2] == 2 * Cn
        out = torch.empty_like(q)
        _lib.check(self.capi, self.capi.i2v_twins_attention_f32(_ptr(q, self), _ptr(kv, self), n, Tq, kv.shape[1], heads, dh,
                                                                dh ** -0.5 if scale is None else scale, _ptr(out, self), self.stream()))
        return out

    def twins_attention_bwd(self, q: torch.Tensor, kv: torch.Tensor, dout: torch.Tensor, heads: int, scale: float = None):
        """The input gradients of that launch (`i2v_twins_attention_bwd_f32`) from dout = d(out): (dq as q, dkv as kv)."""
        n, Tq, Cn = q.shape
        dh = Cn // heads
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        _lib.check(self.capi, self.capi.i2v_twins_attention_bwd_f32(_ptr(q, self), _ptr(kv, self), _ptr(dout, self), n, Tq, kv.shape[1], heads,
                                                                    dh, dh ** -0.5 if scale is None else scale, _ptr(dq, self),
                                                                    _ptr(dkv, self), self.stream()))
        return dq, dkv

    def twins_block_gather(self, x: torch.Tensor, s: int) -> torch.Tensor:
        """The s x s block gather on its own (`i2v_twins_block_gather_f32`): x (n, H, W, C) -> rows (n H/s W/s, s s C)."""
        n, H, W, Cn = x.shape
        rows = torch.empty(n * (H // s) * (W // s), s * s * Cn, dtype=torch.float32, device=x.device)
        _lib.check(self.capi, self.capi.i2v_twins_block_gather_f32(_ptr(x, self), _ptr(rows, self), n, H, W, Cn, s, self.stream()))
        return rows

    def twins_block_scatter(self, drows: torch.Tensor, shape, s: int, into=None) -> torch.Tensor:
        """Its inverse (`i2v_twins_block_scatter_f32`): drows (n H/s W/s, s s C) -> a plane of `shape` (n, H, W, C); `into` is added to."""
        n, H, W, Cn = shape
        dst = into if into is not None else torch.empty(*shape, dtype=torch.float32, device=drows.device)
        _lib.check(self.capi, self.capi.i2v_twins_block_scatter_f32(_ptr(drows, self), _ptr(dst, self), n, H, W, Cn, s, int(into is not None),
                                                                    self.stream()))
        return dst

    def twins_window_attention(self, qkv: torch.Tensor, grid: int, window: int, heads: int, dout: torch.Tensor = None) -> torch.Tensor:
        """Window attention at shift 0 without a table (`i2v_twins_window_attention_f32`; with `dout` its input gradient,
        `i2v_twins_window_attention_bwd_f32`): qkv (frames, grid^2, 3 heads dh) -> out (frames, grid^2, heads dh), or dqkv as qkv."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        zeros = torch.zeros((2 * window - 1) ** 2 * heads, dtype=torch.float32, device=qkv.device)
        if dout is None:
            out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
            _lib.check(self.capi, self.capi.i2v_twins_window_attention_f32(_ptr(qkv, self), n, grid, grid, window, heads, dh, _ptr(zeros, self),
                                                                           _ptr(out, self), self.stream()))
            return out
        dqkv = torch.empty_like(qkv)
        _lib.check(self.capi, self.capi.i2v_twins_window_attention_bwd_f32(_ptr(qkv, self), _ptr(dout, self), n, grid, grid, window, heads, dh,
                                                                           _ptr(zeros, self), _ptr(dqkv, self), self.stream()))
        return dqkv

    def beit_attention(self, qkv: torch.Tensor, bias, heads: int, scale: float = None) -> torch.Tensor:
        """Biased global attention on its own (`i2v_beit_attention_f32`): qkv (frames, T, 3 heads dh), bias (heads, T, T) or None ->
        out (frames, T, heads dh); `scale` defaults to dh^-0.5."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        assert 3 * heads * dh == C3 and (bias is None or tuple(bias.shape) == (heads, T, T))
        out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
        _lib.check(self.capi, self.capi.i2v_beit_attention_f32(_ptr(qkv, self), None if bias is None else _ptr(bias, self), n, T, heads, dh,
                                                               dh ** -0.5 if scale is None else scale, _ptr(out, self), self.stream()))
        return out

    def beit_attention_bwd(self, qkv: torch.Tensor, bias, dout: torch.Tensor, heads: int, scale: float = None) -> torch.Tensor:
        """The input gradient of that launch (`i2v_beit_attention_bwd_f32`) from dout = d(out): dqkv as qkv."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        dqkv = torch.empty_like(qkv)
        _lib.check(self.capi, self.capi.i2v_beit_attention_bwd_f32(_ptr(qkv, self), None if bias is None else _ptr(bias, self), _ptr(dout, self),
                                                                   n, T, heads, dh, dh ** -0.5 if scale is None else scale, _ptr(dqkv, self),
                                                                   self.stream()))
        return dqkv

    def beit_bias_add(self, S: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
        """The bias-add launch of the shared-launch route on its own (`i2v_beit_bias_add_f32`): S (frames, heads, T, ld) += bias
        (heads, T, ld), in place."""
        assert tuple(S.shape[1:]) == tuple(bias.shape)
        _lib.check(self.capi, self.capi.i2v_beit_bias_add_f32(_ptr(S, self), _ptr(bias, self), S.shape[0], bias.numel(), self.stream()))
        return S

    def pit_attention(self, qkv: torch.Tensor, heads: int, scale: float = None):
        """Streaming attention on its own (`i2v_pit_attention_f32`): qkv (frames, T, 3 heads dh), any T -> out (frames, T, heads dh) and the
        row log-sum-exp lse (frames, heads, T); `scale` defaults to dh^-0.5."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        assert 3 * heads * dh == C3
        out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(n, heads, T, dtype=torch.float32, device=qkv.device)
        _lib.check(self.capi, self.capi.i2v_pit_attention_f32(_ptr(qkv, self), n, T, heads, dh, dh ** -0.5 if scale is None else scale,
                                                              _ptr(out, self), _ptr(lse, self), self.stream()))
        return out, lse

    def pit_attention_bwd(self, qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, heads: int,
                          scale: float = None) -> torch.Tensor:
        """The input gradient of that launch (`i2v_pit_attention_bwd_f32`) from the forward's out and lse and dout = d(out): dqkv as qkv."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        dqkv = torch.empty_like(qkv)
        delta = torch.empty_like(lse)
        _lib.check(self.capi, self.capi.i2v_pit_attention_bwd_f32(_ptr(qkv, self), _ptr(out, self), _ptr(lse, self), _ptr(dout, self), n, T, heads,
                                                                  dh, dh ** -0.5 if scale is None else scale, _ptr(delta, self),
                                                                  _ptr(dqkv, self), self.stream()))
        return dqkv

    def pit_pool(self, x: torch.Tensor, w: torch.Tensor, b, grid: int, prefix: int = 0, into: torch.Tensor = None) -> torch.Tensor:
        """The pooling convolution on its own (`i2v_pit_pool_f32`): x (frames, prefix + grid^2, C), w (2 C, 9), b (2 C) or None -> y
        (frames, prefix + go^2, 2 C) whose prefix rows are left as `into` has them (zeros without `into`)."""
        n, T, Cn = x.shape
        go = (grid - 1) // 2 + 1
        assert T == prefix + grid * grid
        y = torch.zeros(n, prefix + go * go, 2 * Cn, dtype=torch.float32, device=x.device) if into is None else into
        _lib.check(self.capi, self.capi.i2v_pit_pool_f32(_ptr(x, self), _ptr(w, self), None if b is None else _ptr(b, self), n, grid, Cn, prefix,
                                                         _ptr(y, self), self.stream()))
        return y

    def pit_pool_bwd(self, dy: torch.Tensor, w: torch.Tensor, grid: int, prefix: int = 0, into: torch.Tensor = None) -> torch.Tensor:
        """Its input gradient (`i2v_pit_pool_bwd_f32`): dy (frames, prefix + go^2, 2 C) -> dx (frames, prefix + grid^2, C), written
        (prefix rows zeros) or, with `into`, added to the grid rows of `into`."""
        n, To, C2 = dy.shape
        dx = torch.zeros(n, prefix + grid * grid, C2 // 2, dtype=torch.float32, device=dy.device) if into is None else into
        _lib.check(self.capi, self.capi.i2v_pit_pool_bwd_f32(_ptr(dy, self), _ptr(w, self), n, grid, C2 // 2, prefix, int(into is not None),
                                                             _ptr(dx, self), self.stream()))
        return dx

    def pit_patch_gather(self, img: torch.Tensor, p: int, s: int) -> torch.Tensor:
        """Overlapping patch rows (`i2v_pit_patch_gather_f32`): img (frames, C, side, side) -> rows (frames g^2, C p^2)."""
        n, Cn, side, _ = img.shape
        g = (side - p) // s + 1
        rows = torch.empty(n * g * g, Cn * p * p, dtype=torch.float32, device=img.device)
        _lib.check(self.capi, self.capi.i2v_pit_patch_gather_f32(_ptr(img, self), n, Cn, side, p, s, _ptr(rows, self), self.stream()))
        return rows

    def pit_patch_scatter(self, rows: torch.Tensor, frames: int, chans: int, side: int, p: int, s: int, into: torch.Tensor = None) -> torch.Tensor:
        """The gather's transpose (`i2v_pit_patch_scatter_f32`): rows -> gimg (frames, C, side, side), written or added to `into`."""
        g = torch.empty(frames, chans, side, side, dtype=torch.float32, device=rows.device) if into is None else into
        _lib.check(self.capi, self.capi.i2v_pit_patch_scatter_f32(_ptr(rows, self), frames, chans, side, p, s, int(into is not None), _ptr(g, self),
                                                                  self.stream()))
        return g

    def coat_attention(self, qkv: torch.Tensor, E: torch.Tensor, heads: int, scale: float = None):
        """Factorized attention on its own (`i2v_coat_factor_attention_f32`): qkv (frames, T, 3 heads dh), E (frames, T, heads dh), any T
        -> out (frames, T, heads dh), gram (frames, heads, dh, dh) and kstat (frames, heads, 2, dh); `scale` defaults to dh^-0.5."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        assert 3 * heads * dh == C3
        out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
        gram = torch.empty(n, heads, dh, dh, dtype=torch.float32, device=qkv.device)
        kstat = torch.empty(n, heads, 2, dh, dtype=torch.float32, device=qkv.device)
        _lib.check(self.capi, self.capi.i2v_coat_factor_attention_f32(_ptr(qkv, self), _ptr(E, self), n, T, heads, dh,
                                                                      dh ** -0.5 if scale is None else scale, _ptr(gram, self),
                                                                      _ptr(kstat, self), _ptr(out, self), self.stream()))
        return out, gram, kstat

    def coat_attention_bwd(self, qkv: torch.Tensor, E: torch.Tensor, gram: torch.Tensor, kstat: torch.Tensor, dout: torch.Tensor, heads: int,
                           scale: float = None):
        """The input gradient of that launch (`i2v_coat_factor_attention_bwd_f32`) from the forward's gram and kstat: dqkv as qkv, and
        dE = dout o q (the crpe backward carries it onto dv)."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        dqkv, dE, dgram = torch.empty_like(qkv), torch.empty_like(E), torch.empty_like(gram)
        _lib.check(self.capi, self.capi.i2v_coat_factor_attention_bwd_f32(_ptr(qkv, self), _ptr(E, self), _ptr(gram, self), _ptr(kstat, self),
                                                                          _ptr(dout, self), n, T, heads, dh,
                                                                          dh ** -0.5 if scale is None else scale, _ptr(dgram, self),
                                                                          _ptr(dqkv, self), _ptr(dE, self), self.stream()))
        return dqkv, dE

    def coat_dwmix(self, x: torch.Tensor, filters, bias, grid: int, prefix: int = 1, residual: bool = False, col: int = 0, channels: int = None,
                   bwd: bool = False, into: torch.Tensor = None, into_col: int = 0) -> torch.Tensor:
        """The per-channel-window depthwise convolution on its own (`i2v_coat_dwmix_f32`, with `bwd` its transpose
        `i2v_coat_dwmix_bwd_f32`): x (frames, prefix + grid^2, row stride) read from column `col` on, `channels` wide (default: the whole
        row); `filters` = (w3, w5, w7) as (9, n3), (25, n5), (49, n7), None for a window without channels -> y (frames, prefix + grid^2, C);
        `into` (backward only): added to instead of written, from its column `into_col` on at its own row stride (dv inside a qkv gradient)."""
        n, T, rs = x.shape
        Cn = rs - col if channels is None else channels
        assert T == prefix + grid * grid
        w3, w5, w7 = filters
        n3, n5 = (0 if w3 is None else w3.shape[1]), (0 if w5 is None else w5.shape[1])
        ptr = lambda t: None if t is None else _ptr(t, self)      # noqa: E731
        y = torch.empty(n, T, Cn, dtype=torch.float32, device=x.device) if into is None else into
        xp, yp = C.c_void_p(_ptr(x, self).value + 4 * col), C.c_void_p(_ptr(y, self).value + 4 * into_col)
        if bwd:
            _lib.check(self.capi, self.capi.i2v_coat_dwmix_bwd_f32(xp, rs, ptr(w3), ptr(w5), ptr(w7), n, grid, Cn, n3, n5, prefix, int(residual),
                                                                   int(into is not None), yp, y.shape[2], self.stream()))
        else:
            _lib.check(self.capi, self.capi.i2v_coat_dwmix_f32(xp, rs, ptr(w3), ptr(w5), ptr(w7), ptr(bias), n, grid, Cn, n3, n5, prefix,
                                                               int(residual), yp, y.shape[2], self.stream()))
        return y

    def coat_cell_gather(self, x: torch.Tensor, grid: int, s: int, prefix: int = 1) -> torch.Tensor:
        """The s x s cells of a token-major plane behind `prefix` rows (`i2v_coat_cell_gather_f32`): x (frames, prefix + grid^2, C) ->
        rows (frames (grid / s)^2, s^2 C)."""
        n, T, Cn = x.shape
        rows = torch.empty(n * (grid // s) ** 2, s * s * Cn, dtype=torch.float32, device=x.device)
        _lib.check(self.capi, self.capi.i2v_coat_cell_gather_f32(_ptr(x, self), n, grid, Cn, s, prefix, _ptr(rows, self), self.stream()))
        return rows

    def coat_cell_scatter(self, rows: torch.Tensor, frames: int, grid: int, s: int, prefix: int = 1, into: torch.Tensor = None) -> torch.Tensor:
        """Its inverse (`i2v_coat_cell_scatter_f32`): rows -> dx (frames, prefix + grid^2, C), written with the prefix rows 0, or added to
        `into`."""
        Cn = rows.shape[1] // (s * s)
        dx = torch.empty(frames, prefix + grid * grid, Cn, dtype=torch.float32, device=rows.device) if into is None else into
        _lib.check(self.capi, self.capi.i2v_coat_cell_scatter_f32(_ptr(rows, self), frames, grid, Cn, s, prefix, int(into is not None),
                                                                  _ptr(dx, self), self.stream()))
        return dx

    def tnt_attention(self, qkv: torch.Tensor, heads: int, scale: float = None) -> torch.Tensor:
        """Attention over many short sequences on its own (`i2v_tnt_attention_f32`): qkv (seqs, T, 3 heads dh), T up to 16, dh up to 16
        (any width), up to 8 heads -> out (seqs, T, heads dh); `scale` defaults to dh^-0.5.  One launch, nothing kept."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        assert 3 * heads * dh == C3
        out = torch.empty(n, T, heads * dh, dtype=torch.float32, device=qkv.device)
        _lib.check(self.capi, self.capi.i2v_tnt_attention_f32(_ptr(qkv, self), n, T, heads, dh, dh ** -0.5 if scale is None else scale,
                                                              _ptr(out, self), self.stream()))
        return out

    def tnt_attention_bwd(self, qkv: torch.Tensor, dout: torch.Tensor, heads: int, scale: float = None) -> torch.Tensor:
        """The input gradient of that launch (`i2v_tnt_attention_bwd_f32`) from qkv and dout alone: dqkv as qkv.  One launch."""
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        dqkv = torch.empty_like(qkv)
        _lib.check(self.capi, self.capi.i2v_tnt_attention_bwd_f32(_ptr(qkv, self), _ptr(dout, self), n, T, heads, dh,
                                                                  dh ** -0.5 if scale is None else scale, _ptr(dqkv, self), self.stream()))
        return dqkv

    def tnt_attention_group(self, T: int, heads: int, dh: int) -> int:
        """Sequences one workgroup of the two launches owns for this shape (`i2v_tnt_attention_group`)."""
        return int(self.capi.i2v_tnt_attention_group(T, heads, dh))

    def tnt_pixel_gather(self, x: torch.Tensor) -> torch.Tensor:
        """The rows of TNT's 7 x 7, stride 4, padding 3 pixel convolution (`i2v_tnt_pixel_gather_f32`): x (frames, C, side, side), side a
        multiple of 16 -> rows (frames (side / 16)^2 16, C 49 rounded up to 4) in (patch, pixel) order."""
        n, Cn, side, _ = x.shape
        rows = torch.empty(n * (side // 4) ** 2, (Cn * 49 + 3) // 4 * 4, dtype=torch.float32, device=x.device)
        _lib.check(self.capi, self.capi.i2v_tnt_pixel_gather_f32(_ptr(x, self), n, Cn, side, _ptr(rows, self), self.stream()))
        return rows

    def tnt_pixel_scatter(self, rows: torch.Tensor, frames: int, in_chans: int, side: int, into: torch.Tensor = None) -> torch.Tensor:
        """Its transpose (`i2v_tnt_pixel_scatter_f32`): rows -> dx (frames, C, side, side), written, or added to `into`."""
        dx = torch.empty(frames, in_chans, side, side, dtype=torch.float32, device=rows.device) if into is None else into
        _lib.check(self.capi, self.capi.i2v_tnt_pixel_scatter_f32(_ptr(rows, self), frames, in_chans, side, int(into is not None),
                                                                  _ptr(dx, self), self.stream()))
        return dx

    # ---- measurement ----
    KINDS = ("conv_igemm_fwd", "conv_igemm_imggrad", "pool_fwd", "pool_bwd", "addmask", "conv_igemm_dgrad")

    def timing_enable(self, on=True):
        """True / 1: one HIP event pair per backbone launch (per-launch times, the low-intensity split, dump lines);
        'segments' / 2: one pair per run of consecutive launches of one kind (a forward list is 3-4 segments: ~2 % less
        overhead on the headline attack, same per-kind totals); False: off."""
        mode = 2 if on in (2, "segments") else (1 if on else 0)
        _lib.check(self.capi, self.capi.i2v_timing_enable(self.h, mode))

    def timing_collect(self):
        """Per kernel kind: device ms, algorithmic flops, launches, algorithmic bytes, and the same over the launches
        whose flops/byte is below the machine balance (`lowi_*`: the HBM-bound ones)."""
        n, f = len(self.KINDS), 8
        out = (C.c_double * (n * f))()
        _lib.check(self.capi, self.capi.i2v_timing_collect_ex(self.h, out, n, f))
        keys = ("ms", "flops", "launches", "bytes", "lowi_ms", "lowi_bytes", "lowi_launches", "lowi_flops")
        return {k: {key: out[i * f + j] for j, key in enumerate(keys)} for i, k in enumerate(self.KINDS)}

    # ---- loop kernels (thin, typed wrappers) ----
    def clip_from_u8(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """(b,t,h,w,3) uint8 decoded frames on the device -> normalised (b,3,t,h,w) float32 clip."""
        assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.shape[-1] == 3
        b, t, h, w, _ = frames_u8.shape
        out = torch.empty(b, 3, t, h, w, dtype=torch.float32, device=frames_u8.device)
        _lib.check(self.capi, self.capi.i2v_clip_from_u8_f32(C.c_void_p(frames_u8.data_ptr()), _ptr(out, self), b, t, h, w, self.stream()))
        return out

    def _quality_api(self):
        """The entries of `include/i2v_quality.h` with their prototypes: `lib.load()` binds them on the product library; an injected
        library (the host simulation) gets them on first use."""
        if not getattr(self, "_quality_bound", False):
            _lib.bind(self.capi, _lib._QUALITY_PROTOS)
            self._quality_bound = True
        return self.capi

    def clip_to_u8(self, video: torch.Tensor, ref: torch.Tensor = None, levels: int = None) -> torch.Tensor:
        """The way back (`i2v_clip_to_u8`): normalised (b,3,t,h,w) float32 clip -> (b,t,h,w,3) uint8 frames, rounded to the nearest level,
        half to even.  With `ref` (the clean clip's frames, same shape) and `levels` the result is also clamped to ref +- levels."""
        assert video.dtype == torch.float32 and video.dim() == 5 and video.shape[1] == 3, (video.dtype, tuple(video.shape))
        b, _, t, h, w = video.shape
        out = torch.empty(b, t, h, w, 3, dtype=torch.uint8, device=video.device)
        if (ref is None) != (levels is None):
            raise _lib.I2VError("clip_to_u8: `ref` and `levels` go together")
        if ref is not None and (ref.dtype != torch.uint8 or tuple(ref.shape) != tuple(out.shape) or ref.device != video.device or not ref.is_contiguous()):
            raise _lib.I2VError(f"clip_to_u8: ref must be contiguous uint8 {tuple(out.shape)} on {video.device}")
        _lib.check(self.capi, self._quality_api().i2v_clip_to_u8(_ptr(video, self), C.c_void_p(ref.data_ptr()) if ref is not None else None,
                                                       -1 if levels is None else int(levels), C.c_void_p(out.data_ptr()), b, t, h, w, self.stream()))
        return out

    def clip_quality_tile(self):
        """(rows, columns) of valid SSIM positions one tile of the quality launch covers (`i2v_clip_quality_tile`)."""
        r, c = C.c_int(), C.c_int()
        self._quality_api().i2v_clip_quality_tile(C.byref(r), C.byref(c))
        return r.value, c.value

    def clip_quality(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """Per frame (SSE in level^2 over 3 h w, max |a - b| in levels, mean SSIM) of two clips on the device, as a float64 (frames, 3)
        tensor: both uint8 (frames..., h, w, 3) -- any leading dimensions -- or both float32 normalised (clips, 3, t, h, w), frame
        clip * t + f (`i2v_clip_quality_u8` / `_f32`).  Nothing synchronises; mixed dtypes or shapes are refused."""
        if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape) or a.device != b.device:
            raise _lib.I2VError(f"clip_quality: operands differ: {a.dtype} {tuple(a.shape)} on {a.device} against {b.dtype} {tuple(b.shape)} on {b.device}")
        if a.device.type != self.device.type or not (a.is_contiguous() and b.is_contiguous()):
            raise _lib.I2VError(f"clip_quality: contiguous tensors on {self.device} needed")
        if a.dtype == torch.uint8 and a.dim() >= 4 and a.shape[-1] == 3:
            h, w = a.shape[-3:-1]
            frames, t = a.numel() // (3 * h * w), 0
        elif a.dtype == torch.float32 and a.dim() == 5 and a.shape[1] == 3:
            clips, _, t, h, w = a.shape
            frames = clips * t
        else:
            raise _lib.I2VError(f"clip_quality: uint8 (..., h, w, 3) frames or float32 (clips, 3, t, h, w) clips, not {a.dtype} {tuple(a.shape)}")
        out = torch.empty(max(frames, 1), 3, dtype=torch.float64, device=a.device)
        nbytes = int(self._quality_api().i2v_clip_quality_scratch_bytes(frames, h, w))
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=a.device)
        pa, pb, po, ps = (C.c_void_p(x.data_ptr()) for x in (a, b, out, scratch))
        if t == 0:
            rc = self.capi.i2v_clip_quality_u8(pa, pb, po, frames, h, w, ps, nbytes, self.stream())
        else:
            rc = self.capi.i2v_clip_quality_f32(pa, pb, po, clips, t, h, w, ps, nbytes, self.stream())
        _lib.check(self.capi, rc)
        if a.device.type == "cuda":          # the scratch goes back to the caching allocator: it must not be handed out to another stream early
            scratch.record_stream(torch.cuda.current_stream(a.device))
        return out[:frames]

    def clip_resize_crop(self, frames_u8: torch.Tensor, short_side=256, crop=224) -> torch.Tensor:
        """(b,t,H,W,3) uint8 decoded frames on the device -> the reference's validation transform (datasets.py:86-93:
        resize the short side to `short_side` with cv2-style 8-bit bilinear, centre-crop `crop`, /255, normalise) ->
        (b,3,t,crop,crop) float32, in one kernel."""
        from . import clips as _clips
        assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.shape[-1] == 3
        b, t, H, W, _ = frames_u8.shape
        rh, rw = _clips.resize_sizes(H, W, short_side)
        cy, cx = _clips.center_crop_origin(rh, rw, crop, crop)
        key = (H, W, rh, rw)
        tabs = self.__dict__.setdefault("_resize_tabs", {})
        if key not in tabs:
            tabs[key] = tuple(torch.from_numpy(_clips.resize_table(n_out, n_in)).to(frames_u8.device) for n_out, n_in in ((rw, W), (rh, H)))
        xt, yt = tabs[key]
        out = torch.empty(b, 3, t, crop, crop, dtype=torch.float32, device=frames_u8.device)
        _lib.check(self.capi, self.capi.i2v_clip_resize_crop_u8_f32(
            C.c_void_p(frames_u8.data_ptr()), _ptr(out, self), C.c_void_p(xt.data_ptr()), C.c_void_p(yt.data_ptr()), b, t, H, W, rh, rw,
            cy, cx, crop, crop, self.stream()))
        return out

    def clip_gather_resize_crop(self, pool: torch.Tensor, offsets, geometry, short_side=256, crop=224) -> torch.Tensor:
        """The validation transform of `clip_resize_crop` over a RAGGED batch in one kernel: clip bi, frame ti is the H*W*3 bytes at
        pool[offsets[bi, ti]:] (pool: uint8, on the device or in host memory -- then uploaded on this engine's stream), each clip
        with its own frame size.  `geometry` is what `clips.kinetics_video_batches` yields -- (geometry int32 (b, 8), xtab, ytab) from
        `clips.gather_geometry` -- or the clips' frame sizes (H, W) (b, 2), from which that is built with `short_side` / `crop`.
        Returns (b,3,t,crop,crop) float32; the library checks every offset and table on the host before it launches."""
        from . import clips as _clips
        import numpy as np
        assert pool.dtype == torch.uint8 and pool.is_contiguous()
        if isinstance(geometry, (tuple, list)) and len(geometry) == 3:
            geom, xtab, ytab = (np.ascontiguousarray(a, np.int32) for a in geometry)
        else:
            geom, xtab, ytab = _clips.gather_geometry(np.asarray(geometry).reshape(-1, 2), short_side, crop)
        offsets = np.ascontiguousarray(offsets, np.int64)
        b, t = offsets.shape
        assert geom.shape == (b, 8) and xtab.ndim == 2 and xtab.shape[1] == 3 and ytab.ndim == 2 and ytab.shape[1] == 3
        if pool.device != self.device:
            pool = pool.to(self.device, non_blocking=True)
        nbytes = int(self.capi.i2v_clip_gather_scratch_bytes(b, t, xtab.shape[0], ytab.shape[0]))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(b, 3, t, crop, crop, dtype=torch.float32, device=self.device)
        _lib.check(self.capi, self.capi.i2v_clip_gather_resize_crop_u8_f32(
            C.c_void_p(pool.data_ptr()), pool.numel(), offsets.ctypes.data_as(C.c_void_p), geom.ctypes.data_as(C.c_void_p), b, t,
            xtab.ctypes.data_as(C.c_void_p), xtab.shape[0], ytab.ctypes.data_as(C.c_void_p), ytab.shape[0], crop, crop, _ptr(out, self),
            C.c_void_p(scratch.data_ptr()), nbytes, self.stream()))
        return out

    def clip_resample_crop(self, frames_u8: torch.Tensor, size=224, crop=224) -> torch.Tensor:
        """(b,t,H,W,3) uint8 decoded frames on the device -> the UCF-101 loader's validation transform (dataset_ucf101.py:113-126:
        PIL BILINEAR `Scale(size)`, `CornerCrop(crop, 'c')`, ToTensor, Normalize) -> (b,3,t,crop,crop) float32, in one kernel."""
        from . import clips as _clips
        assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.shape[-1] == 3
        b, t, H, W, _ = frames_u8.shape
        rh, rw = _clips.scale_sizes(H, W, size)
        cy, cx = _clips.corner_crop_center_origin(rh, rw, crop)
        key = ("pil", H, W, rh, rw)
        tabs = self.__dict__.setdefault("_resize_tabs", {})
        if key not in tabs:
            (xb, xk, kx), (yb, yk, ky) = _clips.pil_resample_table(W, rw), _clips.pil_resample_table(H, rh)
            tabs[key] = tuple(torch.from_numpy(a).to(frames_u8.device) for a in (xb, xk, yb, yk)) + (kx, ky)
        xb, xk, yb, yk, kx, ky = tabs[key]
        out = torch.empty(b, 3, t, crop, crop, dtype=torch.float32, device=frames_u8.device)
        _lib.check(self.capi, self.capi.i2v_clip_resample_crop_u8_f32(
            C.c_void_p(frames_u8.data_ptr()), _ptr(out, self), C.c_void_p(xb.data_ptr()), C.c_void_p(xk.data_ptr()), kx, C.c_void_p(yb.data_ptr()),
            C.c_void_p(yk.data_ptr()), ky, b, t, H, W, rh, rw, cy, cx, crop, crop, self.stream()))
        return out

    def frames_from_video(self, video, x, u):
        b, c, f, h, w = video.shape
        _lib.check(self.capi, self.capi.i2v_frames_from_video_f32(_ptr(video, self), _ptr(x, self), _ptr(u, self), b, f, h, w, self.stream()))

    def compose(self, u, delta, out, b, f, eps, video_layout=False):
        h, w = u.shape[-2:]
        _lib.check(self.capi, self.capi.i2v_compose_f32(_ptr(u, self), _ptr(delta, self), _ptr(out, self), b, f, h, w, eps,
                                                        1 if video_layout else 0, self.stream()))

    def adam_step(self, delta, m, v, gx, u, eps, lr, step_t, beta1=0.9, beta2=0.999, adam_eps=1e-8):
        n, _, h, w = delta.shape
        _lib.check(self.capi, self.capi.i2v_adam_step_f32(_ptr(delta, self), _ptr(m, self), _ptr(v, self), _ptr(gx, self), _ptr(u, self), n, h * w,
                                                          eps, lr, beta1, beta2, adam_eps, step_t, self.stream()))

    def sign_step(self, adv, u, grad, chan_stride, step, eps):
        _lib.check(self.capi, self.capi.i2v_sign_step_f32(_ptr(adv, self), _ptr(u, self), _ptr(grad, self), adv.numel(), chan_stride,
                                                          step, eps, self.stream()))

    def sign_step_delta_gx(self, delta, gx, u, eps, step):
        _lib.check(self.capi, self.capi.i2v_sign_step_delta_gx_f32(_ptr(delta, self), _ptr(gx, self), _ptr(u, self), delta.numel(), eps, step,
                                                                   self.stream()))

    def sign_step_delta(self, delta, grad, step):
        _lib.check(self.capi, self.capi.i2v_sign_step_delta_f32(_ptr(delta, self), _ptr(grad, self), delta.numel(), step, self.stream()))

    def tt_grad_mix(self, grads, kernel, moves, weight):
        """`TemporalTranslation._grad_augmentation` (video_attacks.py:160-175): grads (D, N, C, T, H, W) on the device, kernel /
        moves host sequences of length D -> (N, C, T, H, W)."""
        import numpy as np
        D, N, C_, T, H, W = grads.shape
        k = np.ascontiguousarray(np.asarray(kernel, dtype=np.float32).reshape(D))
        mv = np.ascontiguousarray(np.asarray(moves, dtype=np.int32).reshape(D))
        out = torch.empty(N, C_, T, H, W, dtype=torch.float32, device=grads.device)
        _lib.check(self.capi, self.capi.i2v_tt_grad_mix_f32(_ptr(grads.contiguous(), self), _ptr(out, self), C.c_void_p(k.ctypes.data), C.c_void_p(mv.ctypes.data),
                                                            D, N * C_, T, H * W, float(weight), self.stream()))
        return out

    # ---- base_attacks.py transforms (DI / TI) ----
    def resample_nearest(self, src: torch.Tensor, map_y: torch.Tensor, map_x: torch.Tensor) -> torch.Tensor:
        """dst[..., y, x] = src[..., map_y[y], map_x[x]] (0 where a map is negative); maps: int32 tensors on the device."""
        Hs, Ws = src.shape[-2:]
        out = torch.empty(*src.shape[:-2], map_y.numel(), map_x.numel(), dtype=torch.float32, device=src.device)
        planes = src.numel() // (Hs * Ws)
        _lib.check(self.capi, self.capi.i2v_resample_nearest_f32(_ptr(src, self), _ptr(out, self), planes, Hs, Ws, map_y.numel(), map_x.numel(),
                                                                 C.c_void_p(map_y.data_ptr()), C.c_void_p(map_x.data_ptr()), self.stream()))
        return out

    def resample_nearest_bwd(self, g: torch.Tensor, src_hw, ranges) -> torch.Tensor:
        """Transpose of `resample_nearest`: `ranges` = (ylo, yhi, xlo, xhi) int32 device tensors over the SOURCE rows / columns."""
        Hd, Wd = g.shape[-2:]
        Hs, Ws = src_hw
        out = torch.empty(*g.shape[:-2], Hs, Ws, dtype=torch.float32, device=g.device)
        planes = g.numel() // (Hd * Wd)
        _lib.check(self.capi, self.capi.i2v_resample_nearest_bwd_f32(_ptr(g, self), _ptr(out, self), planes, Hd, Wd, Hs, Ws,
                                                                     *(C.c_void_p(r.data_ptr()) for r in ranges), self.stream()))
        return out

    def dwconv1d(self, src: torch.Tensor, taps, axis: int) -> torch.Tensor:
        """Depthwise 1-D convolution (zero padding, odd len(taps) <= 64) along `axis` of a dense tensor, out of place."""
        import numpy as np
        axis = axis % src.dim()
        k = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
        outer = int(np.prod(src.shape[:axis], dtype=np.int64)) if axis > 0 else 1
        inner = int(np.prod(src.shape[axis + 1:], dtype=np.int64)) if axis + 1 < src.dim() else 1
        out = torch.empty_like(src)
        _lib.check(self.capi, self.capi.i2v_dwconv1d_f32(_ptr(src, self), _ptr(out, self), outer, src.shape[axis], inner,
                                                         C.c_void_p(k.ctypes.data), len(k), self.stream()))
        return out

    GRAD_POST_MODES = {None: 0, "frame": 1, "clip": 2, "column": 3, "l1": 4}

    def grad_post(self, g: torch.Tensor, shape, mode=None, momentum=None, decay=1.0, frame_major=False) -> torch.Tensor:
        """The step between the input gradient and the sign step, fused (`i2v_grad_post_f32`): mean-abs (`'frame'` / `'clip'` /
        `'column'`) or L1 (`'l1'`) normalisation, `+ decay * momentum` with the momentum updated in place, and -- `frame_major` -- the
        change from the backbone's (b*f,c,h,w) gradient to the clip layout.  Returns the (b,c,f,h,w) gradient."""
        b, c, f, h, w = (int(v) for v in shape)
        m = self.GRAD_POST_MODES[mode]
        g = g.contiguous()
        assert g.numel() == b * c * f * h * w, (tuple(g.shape), (b, c, f, h, w))
        assert momentum is None or (momentum.is_contiguous() and tuple(momentum.shape) == (b, c, f, h, w))
        out = torch.empty(b, c, f, h, w, dtype=torch.float32, device=g.device)
        nbytes = int(self.capi.i2v_grad_post_scratch_bytes(b, c, f, h, w, m))
        scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=g.device)
        _lib.check(self.capi, self.capi.i2v_grad_post_f32(_ptr(g, self), _ptr(momentum, self) if momentum is not None else None, _ptr(out, self),
                                                          b, c, f, h, w, 1 if frame_major else 0, m, float(decay), C.c_void_p(scratch.data_ptr()), self.stream()))
        return out

    def tap_perts(self, adv: torch.Tensor, videos: torch.Tensor) -> torch.Tensor:
        """TAP: `(adv - videos) / std` (`base_attacks.py:138-143`, sic), clip layout."""
        b, c, f, h, w = adv.shape
        out = torch.empty_like(adv)
        _lib.check(self.capi, self.capi.i2v_tap_perts_f32(_ptr(adv, self), _ptr(videos, self), _ptr(out, self), b, c, f, h, w, self.stream()))
        return out

    def tap_sign_abs(self, smooth: torch.Tensor, reg_out: torch.Tensor) -> torch.Tensor:
        """TAP: sign(smooth) and, into the one-element `reg_out`, sum|smooth| (`base_attacks.py:731`)."""
        sg = torch.empty_like(smooth)
        scratch = torch.empty(int(self.capi.i2v_tap_scratch_bytes(smooth.numel())), dtype=torch.uint8, device=smooth.device)
        _lib.check(self.capi, self.capi.i2v_tap_sign_abs_f32(_ptr(smooth, self), _ptr(sg, self), _ptr(reg_out, self), smooth.numel(),
                                                            C.c_void_p(scratch.data_ptr()), self.stream()))
        return sg

    def tap_grad(self, gx: torch.Tensor, boxsign: torch.Tensor, weight: float) -> torch.Tensor:
        """TAP: clip-layout gradient = frame-major backbone gradient + weight * boxsign / std."""
        b, c, f, h, w = boxsign.shape
        out = torch.empty_like(boxsign)
        _lib.check(self.capi, self.capi.i2v_tap_grad_f32(_ptr(gx, self), _ptr(boxsign, self), _ptr(out, self), b, c, f, h, w, float(weight), self.stream()))
        return out

    def aens_coeffs(self, prev, coeffs, momentum):
        _lib.check(self.capi, self.capi.i2v_aens_coeffs_f32(_ptr(prev, self), _ptr(coeffs, self), momentum, coeffs.numel(), self.stream()))

    def aens_reduce(self, cos, coeffs, feat_sum, weighted):
        L, n = cos.shape
        _lib.check(self.capi, self.capi.i2v_aens_reduce_f32(_ptr(cos, self), _ptr(coeffs, self), L, n, _ptr(feat_sum, self), _ptr(weighted, self), self.stream()))


# `Engine.build_vit_net`, `build_swin_net`, `build_convnext_net`, `build_mixer_net`, `build_cait_net`, `build_convit_net`, `build_xcit_net`,
# `build_twins_net`, `build_beit_net`, `build_pit_net`, `build_coat_net`, `build_tnt_net`: `build_token_net` under the family's name
for _fam in FAMILIES:
    setattr(Engine, f"build_{_fam.word}_net", Engine.build_token_net)


class HookInfo:
    __slots__ = ("act", "act_stride", "grad", "grad_stride", "D", "post_relu", "shape", "T")


class Net:
    """A planned backbone truncated at its deepest hook."""

    def __init__(self, eng: Engine, graph: Graph, sd, hook_tensors: List[int], max_frames: int, relu_gain=None):
        """`relu_gain`: {ReLU-output tensor of `graph`: backward gain} (`i2v_net_set_relu_gain`; the Skip Gradient Method)."""
        self.eng, capi, h = eng, eng.capi, eng.h
        self.graph = g = graph.truncated(hook_tensors)
        self.max_frames = max_frames
        nid = C.c_int()
        _lib.check(capi, capi.i2v_net_create(h, C.byref(nid)))
        self.id = nid.value
        # buffers / tensors actually referenced
        used_t = {g.input}
        for nd in g.nodes:
            used_t.update([nd.src, nd.dst])
            used_t.update(getattr(nd, "extra_srcs", ()))
            if getattr(nd, "residual", None) is not None:
                used_t.add(nd.residual)
        used_t.update(hook_tensors)
        self.buf_id, self.ten_id = {}, {}
        for t in sorted(used_t):
            ts = g.tensors[t]
            if ts.buf not in self.buf_id:
                out = C.c_int()
                if g.video:
                    _lib.check(capi, capi.i2v_net_add_buffer3d(h, self.id, g.buffers[ts.buf], ts.T, ts.H, ts.W, C.byref(out)))
                else:
                    _lib.check(capi, capi.i2v_net_add_buffer(h, self.id, g.buffers[ts.buf], ts.H, ts.W, C.byref(out)))
                self.buf_id[ts.buf] = out.value
            out = C.c_int()
            _lib.check(capi, capi.i2v_net_add_tensor(h, self.id, self.buf_id[ts.buf], ts.c_off, ts.C,
                                                     1 if ts.post_relu else 0, C.byref(out)))
            self.ten_id[t] = out.value
        _lib.check(capi, capi.i2v_net_set_input(h, self.id, self.ten_id[g.input]))
        for nd in g.nodes:
            if nd.op == "conv":
                w = sd[nd.weight].float().cpu().contiguous()
                scale, shift = fold_affine(nd, sd)
                scale, shift = scale.contiguous(), shift.contiguous()
                if g.video:
                    d = _lib.Conv3dDesc(self.ten_id[nd.src], self.ten_id[nd.dst], nd.cin, nd.cout, nd.kt, nd.kh, nd.kw,
                                        nd.stride_t, nd.stride, nd.pad_t, nd.pad, nd.dil_t, 1 if nd.relu else 0,
                                        -1 if nd.residual is None else self.ten_id[nd.residual])
                    _lib.check(capi, capi.i2v_net_add_conv3d(h, self.id, C.byref(d), _hptr(w), _hptr(scale), _hptr(shift)))
                    continue
                d = _lib.ConvDesc(self.ten_id[nd.src], self.ten_id[nd.dst], nd.cin, nd.cout, nd.kh, nd.kw,
                                  nd.stride, nd.pad, 1 if nd.relu else 0,
                                  -1 if nd.residual is None else self.ten_id[nd.residual])
                if nd.pre_bn:
                    ps, pt = fold_pre_affine(nd, sd)
                    ps, pt = ps.contiguous(), pt.contiguous()
                    _lib.check(capi, capi.i2v_net_add_conv_preact(h, self.id, C.byref(d), _hptr(w), _hptr(scale), _hptr(shift),
                                                                  _hptr(ps), _hptr(pt)))
                elif getattr(nd, "groups", 1) > 1 and nd.groups == nd.cin == nd.cout:        # depthwise
                    _lib.check(capi, capi.i2v_net_add_conv_depthwise(h, self.id, C.byref(d), _hptr(w), _hptr(scale), _hptr(shift)))
                elif getattr(nd, "groups", 1) > 1:
                    _lib.check(capi, capi.i2v_net_add_conv_grouped(h, self.id, C.byref(d), nd.groups, _hptr(w), _hptr(scale), _hptr(shift)))
                else:
                    _lib.check(capi, capi.i2v_net_add_conv(h, self.id, C.byref(d), _hptr(w), _hptr(scale), _hptr(shift)))
            elif nd.op == "se":
                w1 = sd[nd.fc1 + ".weight"].float().cpu().reshape(nd.rd, nd.C).contiguous()
                w2 = sd[nd.fc2 + ".weight"].float().cpu().reshape(nd.C, nd.rd).contiguous()
                b1, b2 = sd[nd.fc1 + ".bias"].float().cpu().contiguous(), sd[nd.fc2 + ".bias"].float().cpu().contiguous()
                d = _lib.SeDesc(self.ten_id[nd.src], self.ten_id[nd.dst], -1 if nd.residual is None else self.ten_id[nd.residual],
                                nd.C, nd.rd, 1 if nd.relu else 0)
                _lib.check(capi, capi.i2v_net_add_se(h, self.id, C.byref(d), _hptr(w1), _hptr(b1), _hptr(w2), _hptr(b2)))
            elif nd.op == "attention":
                d = _lib.AttnDesc(self.ten_id[nd.src], self.ten_id[nd.phi], self.ten_id[nd.g], self.ten_id[nd.dst], float(nd.scale))
                _lib.check(capi, capi.i2v_net_add_attention(h, self.id, C.byref(d)))
            elif g.video:
                d = _lib.Pool3dDesc(self.ten_id[nd.src], self.ten_id[nd.dst], nd.kt, nd.k, nd.stride_t, nd.stride, nd.pad_t, nd.pad)
                _lib.check(capi, capi.i2v_net_add_maxpool3d(h, self.id, C.byref(d)))
            else:
                d = _lib.PoolDesc(self.ten_id[nd.src], self.ten_id[nd.dst], nd.k, nd.stride, nd.pad)
                add = capi.i2v_net_add_avgpool if nd.op == "avgpool" else capi.i2v_net_add_maxpool
                _lib.check(capi, add(h, self.id, C.byref(d)))
        for t, gain in (relu_gain or {}).items():
            if t in self.ten_id:                  # (a ReLU behind the deepest hook is not part of the truncated graph)
                _lib.check(capi, capi.i2v_net_set_relu_gain(h, self.id, self.ten_id[t], float(gain)))
        hooks = (C.c_int * len(hook_tensors))(*[self.ten_id[t] for t in hook_tensors])
        _lib.check(capi, capi.i2v_net_plan(h, self.id, hooks, len(hook_tensors), max_frames))
        self.hook_tensors = hook_tensors
        self.hooks = [self._hook_info(i) for i in range(len(hook_tensors))]

    def _hook_info(self, i) -> HookInfo:
        act, grad = C.c_void_p(), C.c_void_p()
        a_s, g_s, D, pr = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(self.eng.capi, self.eng.capi.i2v_net_hook_info(
            self.eng.h, self.id, i, C.byref(act), C.byref(a_s), C.byref(grad), C.byref(g_s), C.byref(D), C.byref(pr)))
        hi = HookInfo()
        hi.act, hi.act_stride, hi.grad, hi.grad_stride = act.value, a_s.value, grad.value, g_s.value
        hi.D, hi.post_relu = D.value, pr.value
        ts = self.graph.tensors[self.hook_tensors[i]]
        hi.shape = (ts.C, ts.H, ts.W)
        hi.T = ts.T                     # frames per clip at the hook (video backbones)
        return hi

    def close(self):
        """Release the arena and packed weights now (they also go when the engine is destroyed)."""
        if self.id is not None and self.eng.h:
            with self.eng.plan_lock:
                self.eng.capi.i2v_net_destroy(self.eng.h, self.id)
        self.id = None

    def __del__(self):            # an attack object going out of scope gives its arenas back (tens of GB at full size)
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    def workspace_bytes(self) -> int:
        return self.eng.capi.i2v_net_workspace_bytes(self.eng.h, self.id)

    def fusion_info(self):
        """(eligible forward pairs, eligible backward pairs, fused forward pairs, fused backward pairs) of the planned launch lists
        (`i2v_net_fusion_info`): 3x3 convolution + the pointwise convolution over its output as one launch."""
        out = (C.c_int32 * 4)()
        _lib.check(self.eng.capi, self.eng.capi.i2v_net_fusion_info(self.eng.h, self.id, out))
        return tuple(int(v) for v in out)

    def scpair_info(self):
        """(admitted forward pairs, admitted backward pairs, forward pairs run as one launch, backward pairs run as one launch) of the
        planned launch lists (`i2v_net_scpair_info`): a projection shortcut + the expand convolution that adds it as one launch."""
        out = (C.c_int32 * 4)()
        _lib.check(self.eng.capi, self.eng.capi.i2v_net_scpair_info(self.eng.h, self.id, out))
        return tuple(int(v) for v in out)

    def forward(self, x: torch.Tensor):
        _lib.check(self.eng.capi, self.eng.capi.i2v_net_forward(self.eng.h, self.id, _ptr(x, self.eng), x.shape[0], self.eng.stream()))

    def backward(self, gx: torch.Tensor, accumulate=False):
        _lib.check(self.eng.capi, self.eng.capi.i2v_net_backward(self.eng.h, self.id, _ptr(gx, self.eng), 1 if accumulate else 0,
                                                                 self.eng.stream()))

    def read_tensor(self, tid: int, frames: int, grad=False) -> torch.Tensor:
        ts = self.graph.tensors[tid]
        out = torch.empty(frames, ts.C, ts.H, ts.W, dtype=torch.float32, device=self.eng.device)
        _lib.check(self.eng.capi, self.eng.capi.i2v_net_read_tensor(self.eng.h, self.id, self.ten_id[tid], 1 if grad else 0,
                                                                    _ptr(out, self.eng), frames, self.eng.stream()))
        return out

    def save_hook(self, i: int, frames: int) -> torch.Tensor:
        """Detached copy of hook i's feature (the clean `init_feature_maps`, image_attacks.py:319-323)."""
        return self.read_tensor(self.hook_tensors[i], frames)

    def cossim(self, i: int, init: torch.Tensor, cos_out: torch.Tensor, scratch: torch.Tensor, frames: int,
               coef_dev=None, coef_index=0, coef_host=1.0):
        """cos of hook i against its clean feature, gradient written into the hook's gradient view."""
        hi = self.hooks[i]
        capi = self.eng.capi
        _lib.check(capi, capi.i2v_cossim_fwd_bwd_f32(
            C.c_void_p(hi.act), hi.act_stride, _ptr(init, self.eng), hi.D, hi.D, frames,
            C.c_void_p(coef_dev.data_ptr()) if coef_dev is not None else C.c_void_p(0), coef_index, coef_host,
            hi.post_relu, 0, C.c_void_p(cos_out.data_ptr()), C.c_void_p(hi.grad), hi.grad_stride,
            C.c_void_p(scratch.data_ptr()), self.eng.stream()))

    def stdloss(self, i: int, std_out: torch.Tensor, scratch: torch.Tensor, frames: int, exchange=None):
        """Unbiased std of hook i over ALL frames and its gradient.  `exchange(sums, count)` -- given the
        (2,) float64 device tensor of local (sum, sum of squares) and the local element count -- may
        all-reduce the sums in place and return the global count (clip-sharded runs)."""
        hi = self.hooks[i]
        capi = self.eng.capi
        _lib.check(capi, capi.i2v_std_reduce_f32(C.c_void_p(hi.act), hi.act_stride, hi.D, frames,
                                                 C.c_void_p(scratch.data_ptr()), self.eng.stream()))
        total = frames * hi.D
        if exchange is not None:
            total = exchange(scratch[:16].view(torch.float64), total)
        _lib.check(capi, capi.i2v_std_grad_f32(
            C.c_void_p(hi.act), hi.act_stride, hi.D, frames, total, hi.post_relu, 0, C.c_void_p(std_out.data_ptr()),
            C.c_void_p(hi.grad), hi.grad_stride, C.c_void_p(scratch.data_ptr()), self.eng.stream()))

    def hook_frames(self, i: int, in_frames: int) -> int:
        """Frames hook i holds when `in_frames` input frames were run (video backbones change the clip length)."""
        return in_frames // self.graph.tensors[self.graph.input].T * self.hooks[i].T

    def ilaf_scratch_bytes(self, i: int, frames: int, frames_per_seg: int = 0) -> int:
        return self.eng.capi.i2v_ilaf_scratch_bytes(self.hooks[i].D, frames, frames_per_seg)

    def ilaf_reduce(self, i: int, ori: torch.Tensor, adv0: torch.Tensor, scratch: torch.Tensor, frames: int, act=None,
                    frames_per_seg: int = 0):
        """(sum d*d, sum d*d0) of hook i against the dense clean / initial-adversarial feature copies, left as two
        doubles at the start of `scratch`.  `act` overrides the activation (used once to measure |d0|).  `frames_per_seg`:
        independent segments of that many frames (one clip each), two doubles per segment."""
        hi = self.hooks[i]
        capi = self.eng.capi
        a, a_s = (C.c_void_p(hi.act), hi.act_stride) if act is None else (_ptr(act, self.eng), hi.D)
        if frames_per_seg:
            _lib.check(capi, capi.i2v_ilaf_reduce_seg_f32(a, a_s, _ptr(ori, self.eng), _ptr(adv0, self.eng), hi.D, frames, frames_per_seg,
                                                          C.c_void_p(scratch.data_ptr()), self.eng.stream()))
            return
        _lib.check(capi, capi.i2v_ilaf_reduce_f32(a, a_s, _ptr(ori, self.eng), _ptr(adv0, self.eng), hi.D, frames,
                                                  C.c_void_p(scratch.data_ptr()), self.eng.stream()))

    def ilaf_grad(self, i: int, ori, adv0, init_norm, loss_out: torch.Tensor, scratch: torch.Tensor, frames: int,
                  frames_per_seg: int = 0):
        """`init_norm`: |d0| as a host float -- or, with `frames_per_seg`, a DEVICE tensor of float64 holding |d0|^2 per segment;
        `loss_out` then has one element per segment."""
        hi = self.hooks[i]
        capi = self.eng.capi
        if frames_per_seg:
            assert init_norm.dtype == torch.float64 and init_norm.numel() == frames // frames_per_seg
            _lib.check(capi, capi.i2v_ilaf_grad_seg_f32(C.c_void_p(hi.act), hi.act_stride, _ptr(ori, self.eng), _ptr(adv0, self.eng), hi.D, frames,
                                                        frames_per_seg, C.c_void_p(init_norm.data_ptr()), hi.post_relu, 0,
                                                        C.c_void_p(loss_out.data_ptr()), C.c_void_p(hi.grad), hi.grad_stride,
                                                        C.c_void_p(scratch.data_ptr()), self.eng.stream()))
            return
        _lib.check(capi, capi.i2v_ilaf_grad_f32(C.c_void_p(hi.act), hi.act_stride, _ptr(ori, self.eng), _ptr(adv0, self.eng), hi.D, frames,
                                                init_norm, hi.post_relu, 0, C.c_void_p(loss_out.data_ptr()),
                                                C.c_void_p(hi.grad), hi.grad_stride, C.c_void_p(scratch.data_ptr()),
                                                self.eng.stream()))

    def tap_distance(self, i: int, clean: torch.Tensor, coef: float, dist_out: torch.Tensor, scratch: torch.Tensor, frames: int,
                     frames_per_seg: int):
        """TAP's feature-distance term over hook i (`i2v_tap_distance_f32`): per clip || r(a) - r(clean) ||_2 into `dist_out`, and
        coef * its gradient into the hook's gradient view."""
        hi = self.hooks[i]
        _lib.check(self.eng.capi, self.eng.capi.i2v_tap_distance_f32(
            C.c_void_p(hi.act), hi.act_stride, _ptr(clean, self.eng), hi.D, frames, frames_per_seg, float(coef), hi.post_relu, 0,
            C.c_void_p(dist_out.data_ptr()), C.c_void_p(hi.grad), hi.grad_stride, C.c_void_p(scratch.data_ptr()), self.eng.stream()))

    def head_ce(self, i, W: torch.Tensor, bias, labels: torch.Tensor, in_frames: int, scale: float, logits: torch.Tensor,
                loss_each: torch.Tensor, scratch: torch.Tensor):
        """Classifier head over hook i -- or over a LIST of hooks whose pooled features are concatenated in that order
        (SlowFast) -- : global average pool over the clip -> Linear -> cross-entropy, mean over clips, and
        `scale * d loss / d feature` into every hook's gradient view (base_attacks.py:282-284)."""
        capi = self.eng.capi
        clips = in_frames // self.graph.tensors[self.graph.input].T
        bias_p = _ptr(bias, self.eng) if bias is not None else C.c_void_p(0)
        assert labels.dtype == torch.int32 and labels.numel() == clips
        if isinstance(i, int):
            hi = self.hooks[i]
            C_, H_, W_ = hi.shape
            assert W.shape[1] == C_
            _lib.check(capi, capi.i2v_head_ce_f32(
                C.c_void_p(hi.act), hi.act_stride, C_, H_ * W_, hi.T, clips, _ptr(W, self.eng), bias_p,
                W.shape[0], C.c_void_p(labels.data_ptr()), scale, hi.post_relu, 0, _ptr(logits, self.eng), _ptr(loss_each, self.eng), C.c_void_p(hi.grad),
                hi.grad_stride, C.c_void_p(scratch.data_ptr()), self.eng.stream()))
            return
        his = [self.hooks[k] for k in i]
        Ctot = sum(hi.shape[0] for hi in his)
        assert W.shape[1] == Ctot and scratch.numel() >= capi.i2v_head_scratch_bytes(Ctot, clips)
        sp, st = C.c_void_p(scratch.data_ptr()), self.eng.stream()
        off = 0
        for hi in his:
            _lib.check(capi, capi.i2v_head_pool_f32(C.c_void_p(hi.act), hi.act_stride, hi.shape[0], hi.shape[1] * hi.shape[2], hi.T, clips,
                                                    Ctot, off, sp, st))
            off += hi.shape[0]
        _lib.check(capi, capi.i2v_head_logits_ce_f32(Ctot, clips, _ptr(W, self.eng), bias_p, W.shape[0], C.c_void_p(labels.data_ptr()), scale,
                                                     _ptr(logits, self.eng), _ptr(loss_each, self.eng), sp, st))
        off = 0
        for hi in his:
            _lib.check(capi, capi.i2v_head_grad_f32(C.c_void_p(hi.act), hi.act_stride, hi.shape[0], hi.shape[1] * hi.shape[2], hi.T, clips,
                                                    Ctot, off, hi.post_relu, 0, C.c_void_p(hi.grad), hi.grad_stride, sp, st))
            off += hi.shape[0]

    def head_logits(self, i, W: torch.Tensor, bias, in_frames: int, logits: torch.Tensor, scratch: torch.Tensor):
        """Forward-only classifier head (the evaluator, `reference.py:108-129`): global average pool of hook i -- or of a LIST of
        hooks, concatenated in that order -- then `fc`; no loss gradient is written.  `logits`: (clips, K) on the device."""
        capi = self.eng.capi
        his = [self.hooks[k] for k in (i if isinstance(i, (list, tuple)) else [i])]
        clips = in_frames // self.graph.tensors[self.graph.input].T
        Ctot = sum(hi.shape[0] for hi in his)
        assert W.shape[1] == Ctot and scratch.numel() >= capi.i2v_head_scratch_bytes(Ctot, clips)
        sp, st = C.c_void_p(scratch.data_ptr()), self.eng.stream()
        off = 0
        for hi in his:
            _lib.check(capi, capi.i2v_head_pool_f32(C.c_void_p(hi.act), hi.act_stride, hi.shape[0], hi.shape[1] * hi.shape[2], hi.T, clips,
                                                    Ctot, off, sp, st))
            off += hi.shape[0]
        labels = torch.zeros(clips, dtype=torch.int32, device=logits.device)
        loss_each = torch.empty(clips, dtype=torch.float32, device=logits.device)
        bias_p = _ptr(bias, self.eng) if bias is not None else C.c_void_p(0)
        _lib.check(capi, capi.i2v_head_logits_ce_f32(Ctot, clips, _ptr(W, self.eng), bias_p, W.shape[0], C.c_void_p(labels.data_ptr()), 1.0,
                                                     _ptr(logits, self.eng), _ptr(loss_each, self.eng), sp, st))

    def scratch_bytes(self, frames: int) -> int:
        return max(self.eng.capi.i2v_cossim_scratch_bytes(hi.D, frames) for hi in self.hooks)


def token_config(spec):
    """The ctypes config of a transformer surrogate: the struct its family's create entry takes (`lib.family_config`), filled from
    `spec.config_values()` in the struct's order, a sequence padded with zeros to the length of its array field."""
    word = FAMILY_OF[type(spec)].word
    struct = _lib.family_config(word)
    values = list(spec.config_values())
    assert len(values) == len(struct._fields_), (word, len(values))
    for i, (_, ctype) in enumerate(struct._fields_):
        if issubclass(ctype, C.Array):
            v = list(values[i])
            values[i] = ctype(*(v + [0] * (ctype._length_ - len(v))))
    return struct(*values)


class TokenNet(Net):
    """A transformer surrogate behind the `Net` interface the attack loop uses (`forward`, `backward`, `save_hook`, `cossim`, `stdloss`,
    `scratch_bytes`, `hooks`): a hook is a residual stream of `hook_shape(i)[0]` tokens, `hook_shape(i)[1]` wide; the loss kernels are
    the ones every backbone uses.  The family is the spec's row of `graphs.FAMILIES`: its word names the C entries (`i2v_<word>_*`), the
    spec gives the values of the ctypes config (`token_config`) and the weights packed in the family's native order
    (`spec.native_arrays(sd, depth)`, `include/i2v_<word>.h`)."""

    def __init__(self, eng: Engine, spec, sd, hooks: List[int], max_frames: int):
        self.eng, self.graph, self.max_frames, self.id = eng, spec, max_frames, None
        self._api = FAMILY_OF[type(spec)].word
        self.hook_tensors = list(hooks)
        self.h = self._create(spec, sd, self.hook_tensors, max_frames)
        self.hooks = []
        for i in range(len(hooks)):
            act, grad = C.c_void_p(), C.c_void_p()
            a_s, g_s, D = C.c_int64(), C.c_int64(), C.c_int64()
            _lib.check(eng.capi, self._c("hook_info")(self.h, i, C.byref(act), C.byref(a_s), C.byref(grad), C.byref(g_s), C.byref(D)))
            hi = HookInfo()
            hi.act, hi.act_stride, hi.grad, hi.grad_stride, hi.D, hi.post_relu = act.value, a_s.value, grad.value, g_s.value, D.value, 0
            hi.shape, hi.T = self.hook_shape(i), 1
            self.hooks.append(hi)

    def _c(self, name):
        return getattr(self.eng.capi, f"i2v_{self._api}_{name}")

    def _create(self, spec, sd, hooks, max_frames):
        extra = spec.create_extra                       # (between the config and the weight pointers: ViT's prefix count)
        depth = min(max(hooks) + 1, spec.units)         # (a hook outside the blocks / stages is the library's to refuse)
        w = spec.native_arrays(sd, depth)               # kept alive until the upload in the create entry
        ptrs = (C.c_void_p * len(w))(*[t.data_ptr() for t in w])
        cfg = token_config(spec)
        hk = (C.c_int32 * len(hooks))(*hooks)
        h = C.c_void_p()
        _lib.check(self.eng.capi, self._c("create" + ("_ex" if extra else ""))(self.eng.device.index or 0, C.byref(cfg), *extra, ptrs, len(w),
                                                                              hk, len(hooks), max_frames, C.byref(h)))
        return h

    def hook_shape(self, i):
        """(tokens, width, 1) of hook i."""
        return (*self.graph.hook_shape(self.hook_tensors[i]), 1)

    def close(self):
        if getattr(self, "h", None) and self.eng.h:
            with self.eng.plan_lock:
                self._c("destroy")(self.h)
        self.h = None

    def workspace_bytes(self) -> int:
        return int(self._c("workspace_bytes")(self.h))

    def forward(self, x: torch.Tensor):
        spec = self.graph
        if tuple(x.shape[1:]) != (spec.in_chans, spec.img, spec.img):
            raise _lib.I2VError(f"{spec.arch}: frames of shape {tuple(x.shape[1:])}, expected {(spec.in_chans, spec.img, spec.img)}")
        _lib.check(self.eng.capi, self._c("forward")(self.h, _ptr(x, self.eng), x.shape[0], self.eng.stream()))

    def backward(self, gx: torch.Tensor, accumulate=False):
        _lib.check(self.eng.capi, self._c("backward")(self.h, _ptr(gx, self.eng), 1 if accumulate else 0, self.eng.stream()))

    def read_hook(self, i: int, frames: int, grad=False) -> torch.Tensor:
        out = torch.empty(frames, *self.hook_shape(i)[:2], dtype=torch.float32, device=self.eng.device)
        _lib.check(self.eng.capi, self._c("read_hook")(self.h, i, 1 if grad else 0, _ptr(out, self.eng), frames, self.eng.stream()))
        return out

    def save_hook(self, i: int, frames: int) -> torch.Tensor:
        return self.read_hook(i, frames)

    def hook_frames(self, i: int, in_frames: int) -> int:
        return in_frames

