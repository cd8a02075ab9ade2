"""The guards every transformer family's seven C entries share (csrc/i2v_xf.h: xf_create .. xf_read_hook), through each family's own
entries on its test-size twin planned for 2 frames with two hooks: a forward with 0 frames and with one frame too many, a backward before
any forward, hook_info / read_hook of a hook that does not exist, read_hook with too many frames, and a null weights pointer at create.
Every refusal is an I2VError whose text is the entry's own name and the words below, as the planners worded them when each wrote its
own guards.  The host simulation's families run on the CPU; ViT and Swin exist in the device library only."""
import ctypes as C

import pytest
import torch

from i2v_amd import graphs, weights
from i2v_amd import lib as _lib
from tests.hostsim_util import hostsim_engine

MAX_FRAMES = 2
# family word of the entry names -> (model whose twin is planned, its config struct)
FAMILIES = {"vit": ("vit_base_patch16_224", "VitConfig"), "swin": ("swin_tiny_patch4_window7_224", "SwinConfig"),
            "convnext": ("convnext_tiny", "ConvNextConfig"), "mixer": ("mixer_b16_224", "MixerConfig"), "cait": ("cait_xxs24_224", "CaitConfig"),
            "convit": ("convit_tiny", "ConvitConfig"), "xcit": ("xcit_nano_12_p16_224", "XcitConfig"),
            "twins": ("twins_pcpvt_small", "TwinsConfig"), "beit": ("beit_base_patch16_224", "BeitConfig")}
DEVICE_ONLY = ("vit", "swin")


def _refusal(call):
    with pytest.raises(_lib.I2VError) as info:
        call()
    return str(info.value)


def _check_guards(eng, fam):
    model, config = FAMILIES[fam]
    capi = eng.capi
    spec = graphs.build_tiny(model, (64, 64))
    depths = sorted(spec.hooks)
    hooks = [spec.hook_for(depths[0]), spec.hook_for(depths[-1])]
    net = getattr(eng, f"build_{fam}_net")(spec, weights.synthetic_state_dict(spec, 0), hooks, MAX_FRAMES)
    try:
        x = torch.zeros(MAX_FRAMES + 1, 3, 64, 64, device=eng.device)
        gx = torch.zeros_like(x)
        px, pg, s = C.c_void_p(x.data_ptr()), C.c_void_p(gx.data_ptr()), eng.stream()
        out = torch.zeros(MAX_FRAMES + 1, *net.hook_shape(1)[:2], device=eng.device)
        po = C.c_void_p(out.data_ptr())
        check = lambda status: _lib.check(capi, status)      # noqa: E731
        assert _refusal(lambda: check(net._c("backward")(net.h, pg, 0, s))) == f"i2v_{fam}_backward: no forward pass to differentiate"
        for frames in (0, MAX_FRAMES + 1):
            assert _refusal(lambda: check(net._c("forward")(net.h, px, frames, s))) == \
                f"i2v_{fam}_forward: {frames} frames, the net is planned for 1..{MAX_FRAMES}"
        assert _refusal(lambda: check(net._c("backward")(net.h, pg, 0, s))) == f"i2v_{fam}_backward: no forward pass to differentiate"
        n = len(hooks)
        assert _refusal(lambda: check(net._c("read_hook")(net.h, n, 0, po, 1, s))) == f"i2v_{fam}_read_hook: no hook {n}"
        five = [C.byref(t()) for t in (C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64)]
        assert _refusal(lambda: check(net._c("hook_info")(net.h, n, *five))) == f"i2v_{fam}_hook_info: no hook {n}"
        assert _refusal(lambda: check(net._c("read_hook")(net.h, 1, 0, po, MAX_FRAMES + 1, s))) == \
            f"i2v_{fam}_read_hook: {MAX_FRAMES + 1} frames, the net is planned for 1..{MAX_FRAMES}"
        h, hk = C.c_void_p(), (C.c_int32 * 2)(*hooks)
        create = lambda: check(net._c("create")(0, C.byref(getattr(_lib, config)()), None, 4, hk, 2, MAX_FRAMES, C.byref(h)))      # noqa: E731
        assert _refusal(create) == f"i2v_{fam}_create: null argument" and not h.value
        net.forward(x[:1])                                    # the guards left the net usable: one frame, then two
        net.forward(x[:MAX_FRAMES])
        net.backward(gx[:MAX_FRAMES])
        assert tuple(net.read_hook(1, MAX_FRAMES).shape) == (MAX_FRAMES,) + tuple(net.hook_shape(1)[:2])
    finally:
        net.close()


@pytest.mark.parametrize("fam", [f for f in FAMILIES if f not in DEVICE_ONLY])
def test_shared_guards_refuse_in_the_entry_s_own_words(fam):
    eng = hostsim_engine()
    _lib.bind(eng.capi, getattr(_lib, f"_{fam.upper()}_PROTOS"))
    _check_guards(eng, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", DEVICE_ONLY)
def test_shared_guards_refuse_in_the_entry_s_own_words_on_the_device(fam):
    from i2v_amd import attacks
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _check_guards(attacks.get_engine("cuda:0"), fam)
