"""CPU: the 8-bit export and the quality figures (include/i2v_quality.h) on the host simulation, whose entries run
the scalar twins of the launches (csrc/i2v_quality_host.h) -- the arithmetic the MI355X is held to bit for bit (tests/test_gpu_quality.py).

The twins against float64 on the whole table of tests/quality_cases.py, at its bounds; the float64 reference pinned on the smallest
planes by a direct 121-tap loop; the committed taps; identical operands exactly 1.0; the constant pairs' closed form; the checkerboard;
all 768 (level, channel) pairs through `clip_from_u8` and back; the clamp; six wrong references; `quality.summarise`; the refusals; the
three command lines on a tiny net."""
import ctypes as C
import importlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from i2v_amd import lib as _lib
from i2v_amd import quality
from tests import quality_cases as qc
from tests.hostsim_util import hostsim_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32 = qc.fp32_errors()
_REF = {}


def want_of(case):
    """The float64 reference of a case, computed once."""
    if case.name not in _REF:
        a, b = qc.operands(case)
        _REF[case.name] = (a, b, qc.reference(case, a, b))
    return _REF[case.name]


def twin_of(case, _got={}):
    if case.name not in _got:
        a, b, _ = want_of(case)
        _got[case.name] = qc.run_case(hostsim_engine(), case, a, b)
    return _got[case.name]


def test_the_case_table_brackets_the_tile():
    assert hostsim_engine().clip_quality_tile() == (qc.TR, qc.TC)
    text = open(os.path.join(ROOT, "image-to-video-i2v-attack_amd", "csrc", "i2v_quality_kernels.h")).read()
    assert re.search(r"QL_TR = (\d+), QL_TC = (\d+)", text).groups() == (str(qc.TR), str(qc.TC))


@pytest.mark.parametrize("case", qc.SMALLEST, ids=lambda c: c.name)
def test_the_reference_is_the_direct_121_tap_definition(case):
    a, b, want = want_of(case)
    direct = qc.ssim_direct(qc.levels(case, a), qc.levels(case, b))
    assert float((want[:, 2] - direct).abs().max()) < 1e-12


def test_the_committed_taps_are_the_float64_formula_rounded_to_fp32():
    text = open(os.path.join(ROOT, "image-to-video-i2v-attack_amd", "csrc", "i2v_quality_kernels.h")).read()
    body = re.search(r"#define QL_TAP_LITERALS(.*?)\n#define", text, re.S).group(1)
    lits = [np.float32(v) for v in re.findall(r"([0-9.eE+-]+)f", body)]
    want = qc.taps().to(torch.float32).numpy()
    assert len(lits) == 11 and all(a == b for a, b in zip(lits, want)), (lits, want)
    assert [re.search(rf"#define {n} ([0-9.]+) ", text).group(1) for n in ("QL_C1", "QL_C2")] == ["6.5025", "58.5225"]


@pytest.mark.parametrize("case", qc.CASES, ids=lambda c: c.name)
def test_twin_against_float64(case):
    a, b, want = want_of(case)
    got = twin_of(case)
    if case.reps > 1:                                                  # a frame's numbers do not depend on its place in the call
        assert torch.equal(got, got[:want.shape[0]].repeat(case.reps, 1))
        got = got[:want.shape[0]]
    qc.check(case, got, want, FP32)
    if case.content == "same":
        assert torch.equal(got, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64).expand_as(got))           # exactly 1.0
        assert quality.psnr_db(float(got[0, 0]), 3 * case.h * case.w) is None
    if case.content.startswith("const"):
        # the closed form (2ab + C1) / (a^2 + b^2 + C1) per channel, on the levels the operands hold (the f32 mode's are not whole)
        va, vb = qc.levels(case, a)[:, :, 0, 0], qc.levels(case, b)[:, :, 0, 0]
        closed = ((2 * va * vb + qc.C1) / (va * va + vb * vb + qc.C1)).mean(1)
        assert float((want[:, 2] - closed).abs().max()) < 1e-9
        assert float((got[:, 2] - closed).abs().max()) <= qc.bound(FP32[case.name]["ssim"])
    if case.content == "checker":
        assert float(got[:, 2].max()) < -0.9


def test_an_offset_operand_and_a_longer_call_change_nothing():
    for mode in ("u8", "f32"):
        for shape in ("27x13", f"{qc.TR + 11}x{qc.TC + 15}"):
            assert torch.equal(twin_of(qc.BY_NAME[f"{mode}-1x1x{shape}-noise"]), twin_of(qc.BY_NAME[f"{mode}-1x1x{shape}-noise-off1"]))
    five, a = qc.BY_NAME["u8-5x1x27x45-noise"], None
    a, b, _ = want_of(five)
    one = qc.run_case(hostsim_engine(), five._replace(clips=1), a[:1], b[:1])
    assert torch.equal(twin_of(five)[:1], one)


@pytest.mark.parametrize("name", sorted(qc.WRONG))
def test_a_wrong_reference_fails_the_cases_it_must_and_none_it_cannot_change(name):
    kw, must, cannot = qc.WRONG[name]
    seen = set()
    for case in qc.CASES:
        if case.reps > 1 or case.h * case.w > 80 * 80 or not (case.content in must or case.content in cannot):
            continue
        a, b, _ = want_of(case)
        wrong = qc.reference(case, a, b, **kw)
        err = float((twin_of(case)[:, 2] - wrong[:, 2]).abs().max())
        limit = qc.bound(FP32[case.name]["ssim"])
        if case.content in must:
            assert err > limit, (name, case.name, err, limit)
        else:
            assert err <= limit, (name, case.name, err, limit)
        seen.add(case.content)
    assert seen == set(must) | set(cannot)


# ---- the export -----------------------------------------------------------------------------------------------------------------------
def test_all_768_level_channel_pairs_come_back():
    eng = hostsim_engine()
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16, 1).expand(1, 1, 16, 16, 3).contiguous()
    video = eng.clip_from_u8(u8)
    assert torch.equal(video, qc.normalise(u8))
    assert torch.equal(eng.clip_to_u8(video), u8)
    assert torch.equal(qc.run_export(eng, video, offset=1), u8)


def _budget_case(eps):
    """Clean frames over all levels, and the clip the attack's compose step leaves at the edge of the budget: clean +- eps, in [0, 1]."""
    eng = hostsim_engine()
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 2, 8, 16, 1).expand(1, 2, 8, 16, 3).contiguous()
    sign = torch.where(torch.arange(256).view(1, 2, 8, 16, 1) % 2 == 0, 1.0, -1.0)
    unnorm = (u8.to(torch.float32) / 255.0 + sign * eps).clamp(0.0, 1.0)
    mean = torch.tensor(qc.MEAN, dtype=torch.float32).view(1, 1, 1, 1, 3)
    std = torch.tensor(qc.STD, dtype=torch.float32).view(1, 1, 1, 1, 3)
    video = ((unnorm - mean) / std).permute(0, 4, 1, 2, 3).contiguous()
    return eng, u8, video


def test_the_clamp_holds_the_budget_in_levels():
    eng, u8, video = _budget_case(16 / 255)
    assert quality.epsilon_levels(16 / 255) == 16 and quality.epsilon_levels(0.05) == 12 and quality.epsilon_levels(8 / 255) == 8
    plain, held = eng.clip_to_u8(video), eng.clip_to_u8(video, u8, 16)
    assert torch.equal(plain, held)                                                # epsilon 16 / 255 never clamps
    assert int((plain.int() - u8.int()).abs().max()) == 16
    eng, u8, video = _budget_case(0.05)                                            # 12.75 levels: plain rounding gives 13
    plain, held = eng.clip_to_u8(video), eng.clip_to_u8(video, u8, 12)
    assert int((plain.int() - u8.int()).abs().max()) == 13
    assert int((held.int() - u8.int()).abs().max()) == 12
    moved = plain != held
    assert bool(moved.any()) and bool(((held.int() - u8.int()).abs()[moved] == 12).all())
    assert torch.equal(held, qc.run_export(eng, video, u8, 12, offset=1))
    # the ends of the range: level 0 - 12 stays 0, level 255 + 12 stays 255, and values outside [0, 1] or NaN land inside
    wild = video.clone()
    wild[0, :, 0, 0, 0], wild[0, :, 0, 0, 1], wild[0, :, 0, 0, 2] = -100.0, 100.0, float("nan")
    out = eng.clip_to_u8(wild)
    assert out[0, 0, 0, 0].tolist() == [0, 0, 0] and out[0, 0, 0, 1].tolist() == [255, 255, 255] and out[0, 0, 0, 2].tolist() == [0, 0, 0]
    zeros = torch.zeros_like(u8)
    assert int(eng.clip_to_u8(wild, zeros, 12).max()) == 12 and int(eng.clip_to_u8(wild, zeros + 255, 12).min()) == 243
    assert torch.equal(eng.clip_to_u8(video, u8, 0), u8)                           # no budget: the clean frames
    assert torch.equal(eng.clip_to_u8(video, u8, 100000), plain)


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------------
def test_summarise():
    rows = torch.tensor([[3.0, 1.0, 0.5], [9.0, 2.0, 0.7], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    recs = quality.summarise(rows, 2, 4, 5)
    assert recs[0]["psnr_db"] == pytest.approx(10 * math.log10(255 ** 2 / (12.0 / (3 * 2 * 4 * 5))))
    assert recs[0]["ssim"] == pytest.approx(0.6) and recs[0]["linf_levels"] == 2.0
    assert recs[1] == {"psnr_db": None, "ssim": 1.0, "linf_levels": 0.0}
    assert json.loads(json.dumps(recs[1]))["psnr_db"] is None
    assert quality.psnr_db(0.0, 10) is None and quality.psnr_db(65025.0, 1) == pytest.approx(0.0)
    with pytest.raises(ValueError):
        quality.summarise(rows, 3, 4, 5)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def entry_refusals(eng, to_dev=lambda t: t, sync=lambda: None):
    """Every refusal of the entries on `eng`, worded, then a call that works."""
    capi = _lib.bind(eng.capi, _lib._QUALITY_PROTOS)
    case = qc.BY_NAME["u8-1x1x27x13-noise"]
    a, b = (to_dev(t) for t in qc.operands(case))
    fa, fb = (to_dev(t) for t in qc.operands(qc.BY_NAME["f32-1x1x27x13-noise"]))
    out, scratch = to_dev(torch.zeros(3, dtype=torch.float64)), to_dev(torch.zeros(64, dtype=torch.float64))
    P = lambda t: C.c_void_p(t.data_ptr())                                         # noqa: E731
    s, nb = eng.stream(), int(capi.i2v_clip_quality_scratch_bytes(1, 27, 13))
    assert nb == 24 * (-(-17 // qc.TR)) * (-(-3 // qc.TC)) and capi.i2v_clip_quality_scratch_bytes(1, 10, 13) == 0 and capi.i2v_clip_quality_scratch_bytes(0, 27, 13) == 0

    def refused(rc, text):
        assert rc != 0 and text in capi.i2v_last_error().decode(), capi.i2v_last_error()

    u8 = capi.i2v_clip_quality_u8
    refused(u8(None, P(b), P(out), 1, 27, 13, P(scratch), nb, s), "i2v_clip_quality_u8: hipErrorInvalidValue: null argument")
    refused(u8(P(a), None, P(out), 1, 27, 13, P(scratch), nb, s), "null argument")
    refused(u8(P(a), P(b), None, 1, 27, 13, P(scratch), nb, s), "null argument")
    refused(u8(P(a), P(b), P(out), 1, 27, 13, None, nb, s), "null argument")
    refused(u8(P(a), P(b), P(out), 1, 10, 13, P(scratch), nb, s), "smaller than the 11 x 11 window")
    refused(u8(P(a), P(b), P(out), 1, 27, 10, P(scratch), nb, s), "smaller than the 11 x 11 window")
    refused(u8(P(a), P(b), P(out), 0, 27, 13, P(scratch), nb, s), "must be positive")
    refused(u8(P(a), P(b), P(out), -1, 27, 13, P(scratch), nb, s), "must be positive")
    refused(u8(P(a), P(b), P(out), 1, 27, 13, P(scratch), nb - 1, s), "scratch smaller than i2v_clip_quality_scratch_bytes")
    refused(u8(P(a), P(b), P(out), 1, 27, 13, C.c_void_p(scratch.data_ptr() + 4), nb, s), "8-byte aligned")
    f32 = capi.i2v_clip_quality_f32
    refused(f32(None, P(fb), P(out), 1, 1, 27, 13, P(scratch), nb, s), "i2v_clip_quality_f32: hipErrorInvalidValue: null argument")
    refused(f32(P(fa), P(fb), P(out), 0, 1, 27, 13, P(scratch), nb, s), "must be positive")
    refused(f32(P(fa), P(fb), P(out), 1, 0, 27, 13, P(scratch), nb, s), "must be positive")
    refused(f32(P(fa), P(fb), P(out), 1, 1, 27, 13, P(scratch), 0, s), "scratch smaller")
    refused(f32(C.c_void_p(fa.data_ptr() + 1), P(fb), P(out), 1, 1, 27, 13, P(scratch), nb, s), "4-byte alignment")
    frames = to_dev(torch.zeros(1, 1, 27, 13, 3, dtype=torch.uint8))
    to8 = capi.i2v_clip_to_u8
    refused(to8(None, None, -1, P(frames), 1, 1, 27, 13, s), "i2v_clip_to_u8: hipErrorInvalidValue: null argument")
    refused(to8(P(fa), None, -1, None, 1, 1, 27, 13, s), "null argument")
    refused(to8(P(fa), None, -1, P(frames), 0, 1, 27, 13, s), "must be positive")
    refused(to8(P(fa), None, -1, P(frames), 1, 1, 27, 0, s), "must be positive")
    refused(to8(P(fa), P(a), -1, P(frames), 1, 1, 27, 13, s), "a negative budget")
    # the wrapper's own: mixed dtypes, mixed shapes, a budget without its frames
    for x, y in ((a, fa), (a, a[:, :11].contiguous()), (fa, fa[:, :, :, :11].contiguous())):
        with pytest.raises(_lib.I2VError, match="operands differ"):
            eng.clip_quality(x, y)
    with pytest.raises(_lib.I2VError, match="go together"):
        eng.clip_to_u8(fa, levels=3)
    with pytest.raises(_lib.I2VError, match="11 x 11"):
        eng.clip_quality(a[:, :10].contiguous(), b[:, :10].contiguous())
    sync()
    got = eng.clip_quality(a, b)                                                   # the engine goes on
    sync()
    return got.cpu()


def test_refusals_and_the_engine_goes_on():
    case = qc.BY_NAME["u8-1x1x27x13-noise"]
    assert torch.equal(entry_refusals(hostsim_engine()), twin_of(case))


# ---- the command lines ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def tiny_engine(monkeypatch):
    from i2v_amd import attacks, graphs
    eng = hostsim_engine()
    monkeypatch.setitem(attacks._ENGINES, attacks.default_device(), eng)
    monkeypatch.setattr(graphs, "build", graphs.build_tiny)
    return eng


COMMON = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2", "--step_size", "0.005", "--depth", "2",
          "--direction_image_model", "resnet", "--frames", "2", "--hw", "64", "--file_prefix", "t", "--batch_nums", "1", "--batch_index", "1"]
RUN = "Image-ImageGuidedFMDirection_Adam-2-t"


def write_clean_clips(clean_dir, n=2):
    from i2v_amd import clips
    os.makedirs(clean_dir, exist_ok=True)
    for label in range(n):
        np.save(os.path.join(clean_dir, f"{label}-ori.npy"), clips.synthetic_clip(label, 2, 64).numpy())


def check_cli_run(eng, tmp_path, to_dev=lambda t: t, same_bytes=True):
    """`image_main.py` without the flags and with both, `reference.py` on the exported frames, `clip_quality.py` on both directories;
    the engine of the process is `eng`.  `same_bytes`: the second run of the attack repeats the first one's bytes (the host simulation
    does; on the device the planner times its candidates afresh in every run and may settle on another kernel)."""
    import clip_quality
    import image_main
    import reference
    for m in (image_main, reference, clip_quality):
        importlib.reload(m)
    clean_dir = str(tmp_path / "clean")
    write_clean_clips(clean_dir)
    image_main.main(COMMON + ["--clip_dir", clean_dir])
    out = tmp_path / RUN
    plain = sorted(os.listdir(out))
    assert plain == ["0-adv.npy", "1-adv.npy", "loss_info_1.json"]                 # without the flags: the existing contract's files
    before = {f: open(out / f, "rb").read() for f in plain}
    image_main.main(COMMON + ["--clip_dir", clean_dir, "--quality", "--export_u8"])
    assert sorted(os.listdir(out)) == plain + ["quality_info_1.json", "u8"] and sorted(os.listdir(out / "u8")) == ["0-adv.npy", "1-adv.npy"]
    assert not same_bytes or all(open(out / f, "rb").read() == before[f] for f in plain)       # ... and with them, the same bytes
    info = json.load(open(out / "quality_info_1.json"))
    assert sorted(info) == ["0", "1"]
    for label, rec in info.items():
        assert sorted(rec) == ["linf_levels", "psnr_db", "ssim", "u8"] and sorted(rec["u8"]) == ["linf_levels", "psnr_db", "ssim"]
        assert 0 < rec["linf_levels"] <= 16 + 1e-3 and 0 < rec["u8"]["linf_levels"] <= 16
        assert 20 < rec["psnr_db"] < 60 and 0.5 < rec["ssim"] < 1
        frames = np.load(out / "u8" / f"{label}-adv.npy")
        assert frames.dtype == np.uint8 and frames.shape == (2, 64, 64, 3)
        clean = torch.from_numpy(np.load(os.path.join(clean_dir, f"{label}-ori.npy")))
        ref = eng.clip_to_u8(to_dev(clean[None]))
        again = quality.summarise(eng.clip_quality(to_dev(torch.from_numpy(frames)[None].contiguous()), ref).cpu(), 2, 64, 64)[0]
        assert again == rec["u8"]                                                  # ... a recomputation from the written files
        adv = torch.from_numpy(np.load(out / f"{label}-adv.npy"))
        assert quality.summarise(eng.clip_quality(to_dev(adv[None]), to_dev(clean[None])).cpu(), 2, 64, 64)[0] == {k: v for k, v in rec.items() if k != "u8"}
    # clip_quality.py on the run directory and on its u8/ agrees with what the run recorded
    assert clip_quality.main(["--adv_path", RUN, "--clean_dir", clean_dir]) == {k: {f: v[f] for f in v if f != "u8"} for k, v in info.items()}
    assert json.load(open(out / "quality_all_clips.json")) == {k: {f: v[f] for f in v if f != "u8"} for k, v in info.items()}
    assert clip_quality.main(["--adv_path", os.path.join(RUN, "u8"), "--clean_dir", clean_dir]) == {k: v["u8"] for k, v in info.items()}
    # reference.py scores the exported frames: the same predictions as the same clips saved as floats on the grid
    grid = tmp_path / RUN / "grid"
    os.makedirs(grid)
    for label in ("0", "1"):
        frames = torch.from_numpy(np.load(out / "u8" / f"{label}-adv.npy"))
        np.save(grid / f"{label}-adv.npy", qc.normalise(frames[None])[0].numpy())
    acc_u8 = reference.main(["--adv_path", os.path.join(RUN, "u8"), "--models", "i3d_resnet50,tpn_resnet50"])
    acc_f = reference.main(["--adv_path", os.path.join(RUN, "grid"), "--models", "i3d_resnet50,tpn_resnet50"])
    assert acc_u8 == acc_f
    assert open(out / "u8" / "results_all_models_prediction.csv").read() == open(grid / "results_all_models_prediction.csv").read()


def test_the_three_command_lines_on_a_tiny_net(tiny_engine, tmp_path, monkeypatch):
    monkeypatch.setenv("I2V_OPT_PATH", str(tmp_path))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # the engine of this run is the host simulation, whatever the machine has
    check_cli_run(tiny_engine, tmp_path)
