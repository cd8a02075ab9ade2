"""CPU: timm's PiT family as image surrogates on the transformer stack -- for the eight served names the spec, the
hooks and the key / shape contract against tests/golden/timm_pit_keys.json; the refusals; checkpoint loading with a mis-shaped position
table or prefix token refused by key name; the packing (the token-major position table, the (2 C, 9) pool filter) against the reference's
conv2d arithmetic, and that leaving the position table or the pool out, or swapping the prefix tokens, is seen; the kernel entries on the
host simulation, which runs them as scalar code (csrc/i2v_pit_host.h); and the planner itself (csrc/i2v_pit.cpp) on the host simulation:
all three twins against float64, under both routes, and a 4-step I2V attack against the oracle.

The bound is relative L2 against float64: the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets 1e-5)
and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from tests/golden/pit_fp32_cpu_errors.json
(tests/make_pit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import make_pit_fixtures as mk
from tests.family_harness import bound, check_net, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine
from tests.pit_reference import PitReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_pit_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "pit_fp32_cpu_errors.json")))
NAMES = sorted(KEYS["names"])
S, BD = "pit_s_224", "pit_b_distilled_224"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5


def _f(v):
    return None if v is None else v.float().contiguous()


@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._PIT_PROTOS)
    return e


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    assert graphs.build_surrogate(name).param_shapes() == want
    assert KEYS["checked_against"].startswith(("timm ", "unchecked"))


@pytest.mark.parametrize("name", NAMES)
def test_spec_sizes_and_hooks_of_every_name(name):
    patch, stride, base, heads, depths = mk.TABLE[name.replace("_distilled", "")]
    spec = graphs.build_surrogate(name)
    assert isinstance(spec, graphs.PitSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.patch, spec.stride, spec.base_dim, tuple(spec.heads), tuple(spec.depths), spec.ln_eps) == (patch, stride, base, heads, depths, 1e-6)
    assert spec.prefix == (2 if "distilled" in name else 1)
    assert spec.grids == ((31, 16, 8) if patch == 14 else (27, 14, 7)) and spec.widths == tuple(base * h for h in heads)
    d = depths
    assert [spec.hook_for(k) for k in (1, 2, 3, 4)] == [d[0] - 1, d[0] + d[1] // 2 - 1, d[0] + d[1] - 1, sum(d) - 1]
    assert [spec.stage_of(spec.hook_for(k)) for k in (1, 2, 3, 4)] == [0, 1, 1, 2]
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.pit_named(name) == spec and graphs.is_pit_name(name)
    assert not any(f(name) for f in (graphs.is_swin_name, graphs.is_vit_name, graphs.is_beit_name, graphs.is_twins_name, graphs.is_xcit_name))
    assert not any(k.startswith(("head.", "head_dist.", "norm.")) for k in spec.param_shapes())
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224") as ei:
            graphs.build_surrogate(name, hw)
        assert all(n in str(ei.value) for n in NAMES)


def test_hooked_feature_sizes_of_pit_s():
    spec = graphs.build_surrogate(S)
    assert [spec.hook_shape(spec.hook_for(d)) for d in (1, 2, 3, 4)] == [(730, 144), (197, 288), (197, 288), (50, 576)]
    b = graphs.build_surrogate(BD)
    assert b.hook_shape(b.hook_for(1)) == (963, 256) and b.tokens(2) == 66


def test_refusals_name_the_reason_and_list_the_served_names():
    for name in ("pit_s_384", "pit_", "pit_m_224", "pit_s_distilled_384"):
        assert graphs.is_pit_name(name)
        with pytest.raises(ValueError, match="not a model of this table") as ei:
            graphs.build_surrogate(name)
        assert all(n in str(ei.value) for n in NAMES)
        with pytest.raises(ValueError):
            graphs.build_tiny(name)
    assert set(graphs.PIT_MODELS) == set(NAMES) and len(NAMES) == 8


def test_the_resolver_serves_the_names_and_leaves_build_as_it_was():
    """`graphs.build_surrogate` is what the attack classes resolve names with: PiT in front, everything else `graphs.build`'s answer;
    `graphs.build` keeps its vocabulary, where a `pit_*` name is unknown as in the reference."""
    assert graphs.build_surrogate(S) == graphs.pit_named(S) and graphs.build_surrogate("resnet").arch == "resnet101"
    assert isinstance(graphs.build_surrogate("vit_base_patch16_224"), graphs.VitSpec)
    with pytest.raises(UnboundLocalError):
        graphs.build_surrogate("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build(S)
    assert attacks.ImageGuidedFMDirection_Adam([S], depth=1, step_size=0.005, weight_seed=0)._builder is graphs.build_surrogate


def test_test_size_twins():
    t = graphs.build_tiny(S, (64, 64))
    assert t == graphs.build_tiny(BD, (64, 64)) == graphs.pit_tiny_twin()
    assert (t.arch, t.grids, t.prefix, t.base_dim, tuple(t.heads), tuple(t.depths)) == ("pit_test", (7, 4, 2), 1, 16, (2, 4, 8), (2, 2, 2))
    t70 = graphs.build_tiny(S, (70, 70))
    assert (t70.arch, t70.grids, t70.prefix, t70.base_dim, tuple(t70.depths)) == ("pit_test_70", (9, 5, 3), 2, 12, (3, 2, 2)) and t70.base_dim % 16
    t224 = graphs.build_tiny(BD, (224, 224))
    assert (t224.arch, t224.tokens(0), t224.base_dim, tuple(t224.heads), tuple(t224.depths)) == ("pit_test_224", 730, 32, (1, 2, 4), (1, 2, 1))
    assert not any(tw.arch in graphs.PIT_MODELS for tw in (t, t70, t224))
    for hw in ((72, 72), (128, 128), (64, 70)):
        with pytest.raises(ValueError):
            graphs.build_tiny(S, hw)


# ---- checkpoints and packing -------------------------------------------------------------------------------------------------------
def test_checkpoint_loads_and_mis_shaped_tables_are_refused_by_key_name(tmp_path, monkeypatch):
    spec = graphs.build_surrogate("pit_ti_distilled_224")
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match="pit_ti_distilled_224"):
        weights.load_state_dict(spec)
    path = tmp_path / "pit_ti_distilled_224.pth"
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"norm.weight": torch.ones(256), "head.weight": torch.zeros(1).expand(1000, 256), "head_dist.weight": torch.zeros(1).expand(1000, 256)})
    torch.save(sd, path)
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes()) and "head.weight" not in got and "norm.weight" not in got
    torch.save(dict(sd, cls_token=torch.zeros(1, 1, 64)), path)            # a 1-row cls_token under a distilled name
    with pytest.raises(ValueError, match="cls_token"):
        weights.load_state_dict(spec)
    torch.save(dict(sd, pos_embed=torch.zeros(1, 64, 31, 31)), path)        # pit_b's grid
    with pytest.raises(ValueError, match="pos_embed"):
        weights.load_state_dict(spec)
    torch.save(dict(sd, pos_embed=torch.zeros(1, 27 * 27, 64)), path)       # token-major: another layout
    with pytest.raises(ValueError, match="pos_embed"):
        weights.load_state_dict(spec)
    with pytest.raises(weights.MissingWeights):                             # every name reads its own file
        weights.load_state_dict(graphs.build_surrogate("pit_ti_224"))


def test_synthetic_weights_let_the_new_arithmetic_show():
    spec = graphs.build_tiny(S, (70, 70))
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    assert 0.8 < float(sd["pos_embed"].std()) < 1.2 and 0.6 < float(sd["cls_token"].std()) < 1.4
    assert float((sd["cls_token"][0, 0] - sd["cls_token"][0, 1]).abs().mean()) > 0.5
    for s in (0, 1):
        assert 0.25 < float(sd[f"transformers.{s}.pool.conv.weight"].std()) < 0.42


def test_native_arrays_pack_the_position_table_token_major():
    spec = graphs.build_tiny(S, (70, 70))
    sd = weights.synthetic_state_dict(spec, 0)
    w = spec.native_arrays(sd, 4)                                          # three blocks of stage 0, the pool behind it, one block of stage 1
    assert len(w) == 4 + 3 * 12 + 4 + 12 and all(t.dtype == torch.float32 and t.is_contiguous() for t in w)
    pos = w[2]
    assert tuple(pos.shape) == (2 + 81, 24) and float(pos[:2].abs().max()) == 0.0
    assert torch.equal(pos[2 + 9 * 3 + 5], sd["pos_embed"][0, :, 3, 5])
    assert tuple(w[3].shape) == (2, 24) and torch.equal(w[3][1], sd["cls_token"][0, 1])
    assert tuple(w[4 + 36].shape) == (48, 9) and torch.equal(w[4 + 36][7], sd["transformers.0.pool.conv.weight"][7, 0].reshape(9))
    assert len(spec.native_arrays(sd, 3)) == 4 + 36                        # the pool is packed only when the next stage runs


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.PIT_EXPORTS)
    assert {"i2v_pit_attention_f32", "i2v_pit_attention_bwd_f32", "i2v_pit_pool_f32", "i2v_pit_pool_bwd_f32", "i2v_pit_patch_gather_f32",
            "i2v_pit_patch_scatter_f32", "i2v_pit_create"} <= set(_lib.PIT_EXPORTS)
    assert {"i2v_pit.hip", "i2v_pit.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_PIT" in ge.FLAGS
    assert {"i2v_pit_host.h", "i2v_pit_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.PIT_EXPORTS)
    assert "I2V_HAVE_PIT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_pit.h")).read()
    assert all(n + "(" in header for n in _lib.PIT_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_keep_out_and_lse_instead_of_probabilities():
    spec = graphs.build_surrogate(S)
    kern, comp = (spec.workspace_bytes([7], 128, composed=c) for c in (False, True))
    assert 2 ** 31 < kern < comp < 2 ** 38                                                     # past a signed 32-bit count
    F, (T0, T1), (D0, D1), (H0, H1) = 128, (730, 197), (144, 288), (3, 6)
    saves = 2 * (F * T0 * D0 + F * H0 * T0) + 6 * (F * T1 * D1 + F * H1 * T1) + F * H0 * T0      # out and lse per block; delta
    probs = 2 * F * H0 * T0 * 732 + 6 * F * H1 * T1 * 200 + F * H0 * T0 * 732                   # P per block; the score gradient
    assert comp - kern == 4 * (probs - saves)
    assert 4 * 2 * F * H0 * T0 * 732 > 1.6e9                                                    # the 0.8 GB of probabilities per stage-0 block


# ---- the kernel entries on the host simulation (csrc/i2v_pit_host.h) ---------------------------------------------------------------
def run_attn(e, d, dev=lambda t: t):
    qkv = dev(_f(d["qkv"]))
    out, lse = e.pit_attention(qkv, d["heads"])
    dqkv = e.pit_attention_bwd(qkv, out, lse, dev(_f(d["dout"])), d["heads"])
    Cn = dqkv.shape[2] // 3
    return out.cpu(), dqkv[:, :, :Cn].cpu(), dqkv[:, :, Cn:2 * Cn].cpu(), dqkv[:, :, 2 * Cn:].cpu(), lse.cpu()


def check_attn(got, case):
    want = mk.attn_reference(mk.attn_case(*case))
    fp = FP32["attention"][mk.case_key(*case)]
    errs = {"fwd": _rel(got[0], want[0]), "dv": _rel(got[3], want[3]), "lse": _rel(got[4], want[4])}
    if case[1] == 1:      # a single key: dq and dk are identically 0: held absolutely, at rounding of the terms P (dP - delta) ~ 1e-7 |dout . v|
        assert float(got[1].abs().max()) <= 1e-6 and float(got[2].abs().max()) <= 1e-6
    else:
        errs.update({"dq": _rel(got[1], want[1]), "dk": _rel(got[2], want[2])})
    print(f"pit attention {case}: " + ", ".join(f"{k} {v:.3e} (fp32 CPU {fp[k]:.3e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bound(fp[k], FWD_FLOOR if k in ("fwd", "lse") else BWD_FLOOR), (k, v, fp[k])


@pytest.mark.parametrize("case", mk.ATTN_CASES, ids=lambda c: mk.case_key(*c))
def test_attention_entries_on_the_host_simulation(eng, case):
    check_attn(run_attn(eng, mk.attn_case(*case)), case)


def run_pool(e, d, dev=lambda t: t):
    g, pre, go = d["g"], d["prefix"], (d["g"] - 1) // 2 + 1
    x, w = dev(_f(d["x"])), dev(_f(d["w"]).reshape(-1, 9))
    mark = dev(torch.full((x.shape[0], pre + go * go, 2 * x.shape[2]), 7.0))
    y = e.pit_pool(x, w, dev(_f(d["b"])), g, pre, into=mark)
    dy = dev(torch.cat([torch.full((x.shape[0], pre, 2 * x.shape[2]), 9.0), _f(d["dy"])], 1).contiguous())
    dx = e.pit_pool_bwd(dy, w, g, pre)
    base = dev(_f(_rand(*x.shape, seed=11)))
    dxa = e.pit_pool_bwd(dy, w, g, pre, into=base.clone())
    return y.cpu(), dx.cpu(), dxa.cpu(), base.cpu()


def check_pool(res, case):
    y, dx, dxa, base = res
    d = mk.pool_case(*case)
    pre = d["prefix"]
    wy, wdx = mk.pool_reference(d)
    fp = FP32["pool"]["x".join(map(str, case))]
    assert float((y[:, :pre] - 7.0).abs().max() if pre else 0.0) == 0.0     # the prefix rows are skipped, not copied and not cleared
    assert _rel(y[:, pre:], wy) < bound(fp["fwd"], FWD_FLOOR) and _rel(dx[:, pre:], wdx) < bound(fp["bwd"], BWD_FLOOR)
    assert float(dx[:, :pre].abs().max() if pre else 0.0) == 0.0 and torch.equal(dxa[:, :pre], base[:, :pre])
    assert torch.equal(dxa[:, pre:], base[:, pre:] + dx[:, pre:])           # accumulate: the sum formed first, then added once


@pytest.mark.parametrize("case", mk.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_entries_on_the_host_simulation(eng, case):
    check_pool(run_pool(eng, mk.pool_case(*case)), case)


def run_patch(e, d, dev=lambda t: t):
    img, p, s = dev(_f(d["img"])), d["p"], d["s"]
    rows = e.pit_patch_gather(img, p, s)
    n, c, side = img.shape[0], img.shape[1], img.shape[2]
    dr = dev(_f(d["drows"]))
    g = e.pit_patch_scatter(dr, n, c, side, p, s)
    base = dev(_f(_rand(*img.shape, seed=12)))
    ga = e.pit_patch_scatter(dr, n, c, side, p, s, into=base.clone())
    return rows.cpu(), g.cpu(), ga.cpu(), base.cpu()


def check_patch(res, case):
    rows, g, ga, base = res
    d = mk.patch_case(*case)
    wrows, wg = mk.patch_reference(d)
    assert torch.equal(rows, wrows.float())                                 # the gather is a copy
    assert _rel(g, wg) < bound(FP32["patch"]["x".join(map(str, case))]["scatter"], BWD_FLOOR)
    assert torch.equal(ga, base + g)


@pytest.mark.parametrize("case", mk.PATCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_patch_entries_on_the_host_simulation(eng, case):
    check_patch(run_patch(eng, mk.patch_case(*case)), case)


def attention_refusals(e, dev=lambda t: t):
    """dh 6, dh 68, null and misaligned arrays, frames 0: each returns its text, launches nothing and leaves the output untouched."""
    capi = e.capi
    qkv = dev(torch.zeros(1, 8, 3 * 72))
    out, lse = dev(torch.full((1, 8, 72), 5.0)), dev(torch.full((1, 1, 8), 5.0))
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for args, why in (((p(qkv), 1, 8, 1, 6, 1.0, p(out), p(lse)), b"multiple of 4"), ((p(qkv), 1, 8, 1, 68, 1.0, p(out), p(lse)), b"wider than 64"),
                      ((None, 1, 8, 1, 8, 1.0, p(out), p(lse)), b"null argument"), ((p(qkv), 1, 8, 1, 8, 1.0, p(out), None), b"null argument"),
                      ((C.c_void_p(qkv.data_ptr() + 4), 1, 7, 1, 8, 1.0, p(out), p(lse)), b"16-byte alignment"),
                      ((p(qkv), 0, 8, 1, 8, 1.0, p(out), p(lse)), b"must be positive")):
        assert capi.i2v_pit_attention_f32(*args, None) != 0
        msg = capi.i2v_last_error()
        assert why in msg and b"hipErrorInvalidValue" in msg, msg
    dq, delta = dev(torch.full((1, 8, 3 * 8), 5.0)), dev(torch.full((1, 1, 8), 5.0))
    assert capi.i2v_pit_attention_bwd_f32(p(qkv), p(out), p(lse), None, 1, 8, 1, 8, 1.0, p(delta), p(dq), None) != 0
    assert b"null argument" in capi.i2v_last_error()
    assert capi.i2v_pit_attention_bwd_f32(p(qkv), p(out), p(lse), p(out), 1, 8, 1, 6, 1.0, p(delta), p(dq), None) != 0
    assert b"multiple of 4" in capi.i2v_last_error()
    if out.is_cuda:
        torch.cuda.synchronize()
    assert all(float((t.cpu() - 5.0).abs().max()) == 0.0 for t in (out, lse, dq, delta))
    assert capi.i2v_pit_pool_f32(p(qkv), p(qkv), None, 1, 0, 4, 0, p(out), None) != 0 and b"must be positive" in capi.i2v_last_error()
    assert capi.i2v_pit_patch_gather_f32(p(qkv), 1, 3, 11, 4, 3, p(out), None) != 0 and b"do not tile" in capi.i2v_last_error()
    o2, _ = e.pit_attention(dev(torch.zeros(1, 8, 24)), 1)                  # the engine goes on afterwards
    assert float(o2.abs().max()) == 0.0


def test_entry_refusals_on_the_host_simulation(eng):
    attention_refusals(eng)


# ---- the planner (csrc/i2v_pit.cpp) on the host simulation -------------------------------------------------------------------------
def twin_reference(label):
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    ref = PitReference(spec, sd, hooks)
    rf = ref.forward(x)
    hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
    return (spec, sd, x, hooks, rf, hg, ref.backward(hg))


@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, hooks, features, hook gradients, input gradient)."""
    return {label: twin_reference(label) for label in mk.TWINS}


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths and the input gradient with all four hook gradients flowing (a hook behind the last block of stages 0
    and 1 is added where the pooling's gradient lands); a net planned for 5 frames gives the same bits, frame 0 the bits of a 1-frame
    run; every single depth gives the same features and its own gradient."""
    spec, sd, x, hooks, rf, hg, want_gx = twin_refs[label]
    assert spec.arch == label
    feats, gx = _run_twin(eng, spec, sd, hooks, x, hg)
    check_net(label, feats, gx, rf, want_gx, FP32[label], NET_FLOOR)
    f1, g1 = _run_twin(eng, spec, sd, hooks, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    feats2, gx2 = _run_twin(eng, spec, sd, hooks[::-1], x, hg[::-1], max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2[::-1])) and torch.equal(gx, gx2)
    for i in range(4):                                                      # one hook: the net is truncated there
        fa, ga = _run_twin(eng, spec, sd, [hooks[i]], x, [hg[i]])
        assert torch.equal(fa[0], feats[i])
        ref1 = PitReference(spec, sd, [hooks[i]])
        ref1.forward(x)
        assert _rel(ga, ref1.backward([hg[i]])) < bound(FP32[label]["grad"], NET_FLOOR)


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_shared_launch_route_against_float64(eng, twin_refs, label, monkeypatch):
    """I2V_PIT_ATTN=0, read when the net is planned: the core as gemm + softmax + gemm with P kept.  The same bound; the plan holds what
    the formula says under the switch; a net planned without the switch afterwards is the attention launch's again."""
    spec, sd, x, hooks, rf, hg, want_gx = twin_refs[label]
    plain = spec.workspace_bytes(hooks, x.shape[0], composed=False)
    monkeypatch.setenv("I2V_PIT_ATTN", "0")
    feats, gx = _run_twin(eng, spec, sd, hooks, x, hg)                    # (checks the planned bytes against the formula under the switch)
    assert spec.workspace_bytes(hooks, x.shape[0]) != plain
    check_net(label, feats, gx, rf, want_gx, FP32[label], NET_FLOOR)
    monkeypatch.delenv("I2V_PIT_ATTN")
    feats0, gx0 = _run_twin(eng, spec, sd, hooks, x, hg)
    assert all(_rel(a, b) < 1e-5 for a, b in zip(feats, feats0)) and _rel(gx, gx0) < 1e-5


@pytest.mark.parametrize("what", ["pos", "pool", "swap"])
def test_leaving_the_new_arithmetic_out_is_seen(eng, twin_refs, what):
    """The position table, the pool filter and the order of the two prefix tokens carry arithmetic: the reference without the table,
    with a pool filter of zeros, or with the prefix tokens swapped misses a hooked feature of pit_test_70 by more than 100 x its bound
    -- the pool at the depths behind it -- and the library's result through the packing follows the state dict, not the reference's
    shortcut."""
    spec, sd, x, hooks, rf, hg, _ = twin_refs["pit_test_70"]
    feats, _ = _run_twin(eng, spec, sd, hooks, x, hg)
    without = PitReference(spec, sd, hooks, skip=(what,)).forward(x)
    depths = (1, 2, 3) if what == "pool" else (0, 1, 2, 3)
    for i in depths:
        cpu = FP32["pit_test_70"]["hooks"][i]
        assert _rel(without[i], rf[i]) > 100 * bound(cpu, NET_FLOOR) and _rel(feats[i], without[i]) > 100 * bound(cpu, NET_FLOOR)
    blind = dict(sd)                                                       # ... and through the packing: the same state dict with the term changed
    if what == "pos":
        blind["pos_embed"] = torch.zeros_like(sd["pos_embed"])
    elif what == "pool":
        for s in (0, 1):
            blind[f"transformers.{s}.pool.conv.weight"] = torch.zeros_like(sd[f"transformers.{s}.pool.conv.weight"])
    else:
        blind["cls_token"] = sd["cls_token"].flip(1).contiguous()
    fb, _ = _run_twin(eng, spec, blind, hooks, x, hg)
    for i in depths:
        cpu = FP32["pit_test_70"]["hooks"][i]
        assert _rel(fb[i], feats[i]) > 100 * bound(cpu, NET_FLOOR) and _rel(fb[i], without[i]) < bound(cpu, NET_FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(S, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_pit_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_pit_net(spec, sd, [6], 2)
    net = eng.build_pit_net(spec, sd, [1], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    h, one = C.c_void_p(), (C.c_int32 * 1)(0)
    three = lambda *v: (C.c_int32 * 3)(*v)      # noqa: E731
    create = lambda cfg, nw=16: eng.capi.i2v_pit_create(0, C.byref(cfg), (C.c_void_p * nw)(), nw, one, 1, 1, C.byref(h))      # noqa: E731
    assert create(_lib.PitConfig(64, 16, 7, 3, 1, three(32, 64, 128), three(2, 4, 8), three(2, 2, 2), 1e-6)) != 0
    assert b"stride 7" in eng.capi.i2v_last_error()
    assert create(_lib.PitConfig(64, 16, 8, 3, 1, three(136, 272, 544), three(2, 4, 8), three(2, 2, 2), 1e-6)) != 0
    assert b"heads of width 68" in eng.capi.i2v_last_error()
    assert create(_lib.PitConfig(64, 16, 8, 3, 1, three(32, 48, 96), three(2, 4, 8), three(2, 2, 2), 1e-6)) != 0
    assert b"twice its predecessor" in eng.capi.i2v_last_error()
    assert create(_lib.PitConfig(64, 16, 8, 3, 3, three(32, 64, 128), three(2, 4, 8), three(2, 2, 2), 1e-6)) != 0
    assert b"prefix tokens 3" in eng.capi.i2v_last_error()
    assert create(_lib.PitConfig(64, 16, 8, 3, 1, three(32, 64, 128), three(2, 4, 8), three(2, 2, 2), 1e-6), 15) != 0
    assert b"15 weight arrays given, 16 expected" in eng.capi.i2v_last_error()


def test_attack_classes_and_the_command_line_take_the_names(tmp_path, monkeypatch):
    attacks.ImageGuidedFMDirection_Adam([S, "resnet50", "vit_base_patch16_224"], depth=3, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedStd_Adam([BD], depth=1, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedFML2_Adam_MultiModels([S, "resnet50", "vit_base_patch16_224"], depths={S: 2, "resnet50": 3, "vit_base_patch16_224": 2}, weight_seed=0)
    attacks.AENS_I2V_MF([BD, "resnet50"], depths={BD: [2, 4], "resnet50": [2, 3]}, step_size=0.005, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([S], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="not a model of this table") as ei:
        attacks.ImageGuidedFMDirection_Adam(["pit_s_384"], depth=2, step_size=0.005, weight_seed=0)
    assert all(n in str(ei.value) for n in NAMES)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in NAMES:
        for depth in ("1", "2", "3", "4"):
            a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", depth])
            assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "pit_s_384"], ["--direction_image_model", S, "--depth", "5"],
                ["--direction_image_model", S, "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_i2v_trajectory_on_the_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 3 (one pooling passed) against `restate.run_attack` on the float32 reference net (costs at
    rtol 2e-4, as tests/test_beit_cpu.py)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([S], depth=3, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(S, (64, 64))
    check_trajectory(atk, adv, PitReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(3)], dtype=torch.float32), vid, rtol=2e-4, steps=4)
