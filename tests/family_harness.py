"""What the tests of the transformer surrogate families share: seeded inputs, the error measure and its bound,
the reference class around a family's `streams` function, the two ways of feeding hook gradients to a planned net, and the run /
compare steps of the net tests, on the MI355X and on the host simulation alike.  A family's test files keep their own facts as data (the
launch counter, the launches per block, the floors, the trajectory tolerance) and their kernel-entry cases and refusals as code."""
import ctypes as C
import inspect
import os
from typing import Sequence

import numpy as np
import torch

from oracle import restate


def rel(a, b):
    """Relative L2 error of `a` against `b`, in float64 on the host."""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def rand(*shape, seed=0, scale=1.0):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return t if scale == 1.0 else t * scale


def bound(fp32_err, floor):
    """The larger of the floor for that kind of case and 4 x the float32 CPU run's own error against float64."""
    return max(floor, 4.0 * fp32_err)


def video(b, f, hw, seed):
    """A clip batch (b, 3, f, hw, hw) drawn as uint8 and normalised as the loader normalises it."""
    gen = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (b, 3, f, hw, hw), generator=gen, dtype=torch.uint8)
    mean = torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    return (u8.float() / 255 - mean) / std


def stat(eng, name):
    return int(eng.capi.i2v_backend_stat(name))


# ---- the float64 reference around a family's arithmetic -------------------------------------------------------------------------------
class StreamsReference:
    """The interface `oracle.restate.run_attack` drives (`.dtype`, `.hooks`, `forward` -> the hooked features as (frames, D), `backward`
    of hook gradients -> the input gradient by autograd) around a family's `streams(x, state dict, spec, n, **switches)`: the streams
    behind hooks 0 .. n - 1, each frames first.  A family's class is a subclass that names its function
    (`class TntReference(StreamsReference): streams = staticmethod(streams)`).  The switches (`skip=` and kin: what the sensitivity checks
    leave out) are `streams`' own keywords; one it does not have is refused here."""
    streams = None

    def __init__(self, spec, state_dict, hooks: Sequence[int], dtype=torch.float64, device="cpu", **switches):
        unknown = set(switches) - set(inspect.signature(self.streams).parameters)
        if unknown:
            raise TypeError(f"{type(self).__name__}: no switch {sorted(unknown)}")
        self.spec, self.dtype, self.device = spec, dtype, torch.device(device)
        self.hooks = list(hooks)
        self.sd = {k: v.to(dtype).to(self.device) for k, v in state_dict.items()}
        self.switches = switches
        self._x = self._feats = None

    def forward(self, x: torch.Tensor):
        self._x = x.detach().to(self.dtype).to(self.device).requires_grad_(True)
        outs = self.streams(self._x, self.sd, self.spec, max(self.hooks) + 1, **self.switches)
        self._feats = [outs[k].reshape(x.shape[0], -1) for k in self.hooks]
        return [f.detach() for f in self._feats]

    def backward(self, hook_grads: Sequence[torch.Tensor]) -> torch.Tensor:
        g = torch.autograd.grad(self._feats, self._x, [h.to(self.dtype).to(self.device) for h in hook_grads])[0]
        return g.detach()


# ---- hook gradients, written where the loss kernels would write them ------------------------------------------------------------------
def _hip():
    for path in (os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"), "libamdhip64.so"):
        try:
            return C.CDLL(path)
        except OSError:
            continue
    raise OSError("libamdhip64.so not found")


def _set_hook_grads(net, hg):
    """On the device: one device-to-device copy per hook into its gradient view."""
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for hi, g in zip(net.hooks, hg):
        gd = g.float().cuda().contiguous()
        assert gd.numel() == g.shape[0] * hi.D
        torch.cuda.synchronize()
        assert hip.hipMemcpy(hi.grad, gd.data_ptr(), gd.numel() * 4, 3) == 0       # device to device


def write_hook_grads(net, hg):
    """On the host simulation: one copy per frame, `grad_stride` floats apart."""
    for hi, g in zip(net.hooks, hg):
        flat = g.float().reshape(g.shape[0], -1).contiguous()
        for n in range(flat.shape[0]):
            C.memmove(hi.grad + 4 * n * hi.grad_stride, flat[n].data_ptr(), 4 * hi.D)


def hook_width(spec, hook):
    """Floats per frame behind `hook`, as the family's spec states it: `hook_dim` (a method of the hook, or one figure), `hook_shape`
    (PiT, CoaT-Lite: tokens and width), or tokens x dim (plain ViT)."""
    if hasattr(spec, "hook_dim"):
        return spec.hook_dim(hook) if callable(spec.hook_dim) else spec.hook_dim
    if hasattr(spec, "hook_shape"):
        return spec.hook_shape(hook)[0] * spec.hook_shape(hook)[1]
    return spec.tokens * spec.dim


# ---- a planned net: run it, compare it ------------------------------------------------------------------------------------------------
def run_net(net, spec, hooks, x, hg=None, device="cuda"):
    """Forward, the hooked features, hook gradients in (drawn with seeds 30 + i where none are given), backward: (features, input
    gradient, hook gradients), on the host.  Every hook's width is held against the net's own and the spec's."""
    on_gpu = device != "cpu"
    xd = x.float().cuda() if on_gpu else x.float().contiguous()
    net.forward(xd)
    n = x.shape[0]
    feats = [net.save_hook(i, n).reshape(n, -1) for i in range(len(hooks))]
    assert all(f.shape[1] == hook_width(spec, h) == hi.D for f, h, hi in zip(feats, hooks, net.hooks))
    if hg is None:
        hg = [rand(*f.shape, seed=30 + i) for i, f in enumerate(feats)]
    if on_gpu:
        torch.cuda.synchronize()
        _set_hook_grads(net, hg)
    else:
        write_hook_grads(net, hg)
    gx = torch.empty_like(xd)
    net.backward(gx)
    if on_gpu:
        torch.cuda.synchronize()
    return [f.cpu() for f in feats], gx.cpu(), hg


def hooks_and_grad(eng, spec, sd, hooks, x, max_frames=None, launches=None, hg=None, device="cuda", **route):
    """A net planned for `max_frames` frames (default: those of `x`), its workspace held against the spec's formula (`route`: the
    formula's `composed=` where the test names the route), run once and closed: ((features, input gradient), hook gradients).
    `launches` = (counter name, count): what the run must add to that counter."""
    frames = max_frames or x.shape[0]
    net = eng.build_token_net(spec, sd, hooks, frames)
    assert net.workspace_bytes() == spec.workspace_bytes(hooks, frames, **route)
    s0 = stat(eng, launches[0]) if launches else 0
    feats, gx, hg = run_net(net, spec, hooks, x, hg, device)
    if launches:
        assert stat(eng, launches[0]) - s0 == launches[1]
    net.close()
    return (feats, gx), hg


def run_twin(eng, spec, sd, hooks, x, hg, max_frames=None):
    """`hooks_and_grad` on the host simulation with the hook gradients given: (features, input gradient)."""
    return hooks_and_grad(eng, spec, sd, hooks, x, max_frames, hg=hg, device="cpu")[0]


def check_net(label, feats, gx, rf, want_gx, fp32, floor):
    """Features and input gradient against the float64 reference's, each within `bound` of the float32 CPU run's recorded error."""
    errs, gerr = [rel(a, b) for a, b in zip(feats, rf)], rel(gx, want_gx)
    print(f"{label} vs float64: hooks {errs} grad {gerr}; fp32 CPU: {fp32['hooks']} {fp32['grad']}")
    for e, cpu in zip(errs, fp32["hooks"]):
        assert e < bound(cpu, floor)
    assert gerr < bound(fp32["grad"], floor)


def check_trajectory(atk, adv, reference, vid, rtol, steps=10):
    """The costs of the I2V attack `atk` has run on `vid` against the trajectory of `restate.run_attack` over `reference` within `rtol`,
    and, where the test hands them over, the clips it returned against the reference's."""
    ref = restate.run_attack([reference], vid, steps=steps, step_size=0.005)
    print("costs", atk.last_costs, "reference", ref["costs"], "rtol", rtol)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=rtol)
    if adv is not None:
        assert float((adv.cpu() - ref["adv"].float()).abs().mean()) < 5e-3
