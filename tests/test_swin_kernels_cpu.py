"""The window-attention and patch-merging case table (tests/swin_cases.py) on the CPU.  The two launches have no host twin, so nothing
here runs a kernel; what is checked is that the table can tell a wrong kernel from a right one:

  * the reference's shift mask against the brute-force seam test at every (H, W, ws, shift) of the table;
  * the committed float32 fixture: its ids and names, and three cases recomputed;
  * the condition that makes the `hot` cases worth having: there, adding -100 and excluding the key are different functions;
  * sensitivity: each wrong variant of the float64 reference -- a plausible slip in the kernel's index arithmetic -- is fed to `check` as
    what the device returned; the cases it must break fail, and every case it leaves alone still passes."""
import pytest
import torch

from tests import swin_cases as sc
from tests import swin_reference as sr
from tests.make_swin_kernel_fixtures import compute, load

E32 = load()
WIN = {c.id: c for c in sc.WIN_CASES}


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_the_table_takes_the_branches_its_docstring_names():
    n = {c.id: sc.nprob(c.kw) for c in sc.WIN_CASES}
    assert (n["win-f1-7x7-ws7-s0-h1"], n["win-f1-7x7-ws7-s0-h3"], n["win-f1-7x14-ws7-s0-h5"], n["win-f1-14x21-ws7-s3-h1"]) == (1, 3, 10, 6)
    assert (n["win-f1-21x14-ws7-s6-h3"], n["win-f1-4x4-ws4-s0-h1"], n["win-f5-4x8-ws4-s0-h1"]) == (18, 1, 10)
    assert {v % 4 for v in n.values()} == {0, 1, 2, 3} and {v % 2 for v in n.values()} == {0, 1}          # every count of spare waves
    kws = [c.kw for c in sc.WIN_CASES]
    for ws in (7, 4):
        shifts = {k["shift"] for k in kws if k["ws"] == ws}
        assert {0, 1, ws // 2, ws - 1} <= shifts, (ws, shifts)
        assert {(k["H"] > k["W"]) - (k["H"] < k["W"]) for k in kws if k["ws"] == ws and k["shift"]} == {-1, 0, 1}
        assert any(k["H"] < k["W"] for k in kws if k["ws"] == ws) and any(k["H"] > k["W"] for k in kws if k["ws"] == ws)
    assert any(k["H"] // k["ws"] >= 2 and k["W"] // k["ws"] >= 3 and k["shift"] for k in kws)              # an interior window column: all nine regions
    assert {k["kind"] for k in kws} == {"plain", "hot", "notable"} and any(k["heads"] % 2 and k["heads"] > 1 for k in kws)
    f, H, W, C = sc.MERGE_BIG
    quads = f * H * W * C // 4
    assert quads == 16777352 and quads - sc.MERGE_CAP == 136
    assert all(c.kw["frames"] * c.kw["H"] * c.kw["W"] * c.kw["C"] // 4 <= sc.MERGE_CAP for c in sc.MERGE_CASES)
    assert {c.kw["C"] for c in sc.MERGE_CASES} >= {4, 96} and any(c.kw["H"] != c.kw["W"] for c in sc.MERGE_CASES)


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_inputs_are_finite_and_the_reference_passes_its_own_check(case):
    inp = sc.inputs(case)
    assert all(bool(torch.isfinite(t).all()) for t in inp.values())
    if case.op == "win":
        kind = case.kw["kind"]
        assert float(inp["qkv"].std()) == pytest.approx(sc.QKV_SCALE * (sc.HOT if kind == "hot" else 1), rel=0.1)
        assert bool(inp["table"].any()) != (kind == "notable")
    sc.check(case, sc.as_got(sc.reference(case)), E32.get(case.id, {}))
    spoilt = sc.as_got(sc.reference(case))
    name = next(n for n in spoilt if n.endswith("_slack"))
    spoilt[name][-1] = 0.0                                        # one float past the tail
    with pytest.raises(AssertionError):
        sc.check(case, spoilt, E32.get(case.id, {}))


# ---- the reference, where the new cases take it -------------------------------------------------------------------------------------
GEOMETRIES = sorted({(c.kw["H"], c.kw["W"], c.kw["ws"], c.kw["shift"]) for c in sc.WIN_CASES if c.kw["shift"]})


@pytest.mark.parametrize("H,W,ws,shift", GEOMETRIES)
def test_mask_equals_the_brute_force_region_test(H, W, ws, shift):
    """tests/test_swin_cpu.py's seam test with H and W apart: two tokens of a window of the rolled grid may attend to each other exactly
    when neither axis wraps between them -- both on the same side of the seam at rolled row H - shift, and of the one at column W - shift."""
    m = sr.shift_mask(H, W, ws, shift)
    nwy, nwx = H // ws, W // ws
    assert m.shape == (nwy * nwx, ws * ws, ws * ws)
    for wy in range(nwy):
        for wx in range(nwx):
            for i in range(ws * ws):
                for j in range(ws * ws):
                    yi, xi, yj, xj = wy * ws + i // ws, wx * ws + i % ws, wy * ws + j // ws, wx * ws + j % ws
                    same = ((yi >= H - shift) == (yj >= H - shift)) and ((xi >= W - shift) == (xj >= W - shift))
                    assert float(m[wy * nwx + wx, i, j]) == (0.0 if same else -100.0), (wy, wx, i, j)
    assert bool((m[-1] != 0).any()) and (nwy < 2 or nwx < 2 or not bool(m[0].any()))


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_the_table_and_three_cases_recompute():
    assert set(E32) == set(WIN)
    assert all(tuple(v) == sc.WIN_OUTPUTS for v in E32.values())
    ids = ("win-f1-4x4-ws4-s0-h1", "win-f1-14x21-ws7-s3-h1", "win-f1-14x14-ws7-s3-h2-hot")
    assert compute(ids) == {i: E32[i] for i in ids}
    ordinary = [v for k, v in E32.items() if not k.endswith("-hot")]
    assert all(5e-8 < e < 2e-6 for v in ordinary for e in v.values())


# ---- the switches: a local copy of swin_reference.window_attention ------------------------------------------------------------------
def _attention(swap_hw=False, roll_one_axis=False, mask_rows_only=False, mask_value=-100.0, bias_transposed=False, next_head=False,
               no_roll_back=False):
    def mask(H, W, ws, shift, dtype):
        img = torch.zeros(1, H, W, 1, dtype=dtype)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hs, wsl, :] = cnt
                cnt += 0 if mask_rows_only else 1
            cnt += 1 if mask_rows_only else 0
        mw = sr.window_partition(img, ws).reshape(-1, ws * ws)
        diff = mw[:, None, :] - mw[:, :, None]
        return torch.where(diff != 0, torch.full_like(diff, mask_value), torch.zeros_like(diff))

    def attention(qkv, H, W, ws, shift, heads, table):
        N, T, C3 = qkv.shape
        C = C3 // 3
        dh = C // heads
        gh, gw = (W, H) if swap_hw else (H, W)                                       # the grid as the roll and the partition take it
        dims = (1,) if roll_one_axis else (1, 2)
        g = qkv.reshape(N, gh, gw, C3)
        if shift:
            g = torch.roll(g, shifts=(-shift,) * len(dims), dims=dims)
        w = sr.window_partition(g, ws)
        B, n = w.shape[0], ws * ws
        q, k, v = w.reshape(B, n, 3, heads, dh).permute(2, 0, 3, 1, 4)
        att = (q * dh ** -0.5) @ k.transpose(-2, -1)
        idx = sr.relative_position_index(ws)
        bias = table[(idx.t() if bias_transposed else idx).reshape(-1)].reshape(n, n, heads).permute(2, 0, 1)
        if next_head:
            bias = torch.roll(bias, -1, 0)                                           # head h reads table column (h + 1) % heads
        att = att + bias.unsqueeze(0)
        if shift:
            m = mask(H, W, ws, shift, qkv.dtype)
            att = (att.reshape(B // m.shape[0], m.shape[0], heads, n, n) + m[None, :, None]).reshape(B, heads, n, n)
        o = (torch.softmax(att, -1) @ v).transpose(1, 2).reshape(B, n, C)
        o = sr.window_reverse(o, ws, gh, gw)
        if shift and not no_roll_back:
            o = torch.roll(o, shifts=(shift,) * len(dims), dims=dims)
        return o.reshape(N, T, C)
    return attention


def test_the_local_copy_without_a_switch_is_the_reference():
    for case in sc.WIN_CASES:
        ref, mine = sc.reference(case), sc.evaluate(case, attention=_attention())
        assert all(torch.equal(ref[n][1], mine[n][1]) for n in ref), case.id


@pytest.mark.parametrize("case", sc.HOT_CASES, ids=[c.id for c in sc.HOT_CASES])
def test_hot_cases_tell_adding_minus_100_from_excluding_the_key(case):
    """A condition on the inputs, not a measurement of a kernel: with -1e30 for -100 the float64 reference moves by more than 1e-3 of
    max|out| in at least 10 token rows.  (At the ordinary magnitude it moves in none: see the sensitivity test.)"""
    want = sc.reference(case)["out"][1]
    excl = sc.evaluate(case, attention=_attention(mask_value=-1e30))["out"][1]
    rows = int(((want - excl).abs().amax(-1) > 1e-3 * float(want.abs().max())).sum())
    print(f"{case.id}: {rows} of {want.shape[0] * want.shape[1]} rows differ")
    assert rows >= 10
    cold = sc.BY_ID[case.id[:-len("-hot")]] if case.id[:-len("-hot")] in sc.BY_ID else None
    if cold is not None:
        a, b = sc.reference(cold)["out"][1], sc.evaluate(cold, attention=_attention(mask_value=-1e30))["out"][1]
        assert float((a - b).abs().max()) < 1e-12 * float(a.abs().max())


# ---- sensitivity: the table must bite -----------------------------------------------------------------------------------------------
def _ids(pred):
    return {c.id for c in sc.WIN_CASES if pred(c.kw)}


SHIFTED = _ids(lambda k: k["shift"] != 0)
UNSHIFTED = set(WIN) - SHIFTED
WITH_TABLE = _ids(lambda k: k["kind"] != "notable")
# switch -> (the cases that must fail, the cases the switch cannot change, which must still pass)
VARIANTS = {
    "swap_hw": (_ids(lambda k: k["H"] != k["W"]), _ids(lambda k: k["H"] == k["W"])),
    "roll_one_axis": (SHIFTED, UNSHIFTED),
    "mask_rows_only": (SHIFTED, UNSHIFTED),
    "mask_value": ({c.id for c in sc.HOT_CASES}, UNSHIFTED),
    "bias_transposed": (WITH_TABLE, set(WIN) - WITH_TABLE),
    "next_head": (_ids(lambda k: k["heads"] > 1 and k["kind"] != "notable"), _ids(lambda k: k["heads"] == 1 or k["kind"] == "notable")),
    "no_roll_back": (SHIFTED, UNSHIFTED),
}


@pytest.mark.parametrize("switch", sorted(VARIANTS))
def test_a_wrong_window_attention_fails_the_table(switch):
    must_fail, unaffected = VARIANTS[switch]
    assert must_fail and unaffected and not must_fail & unaffected
    wrong = _attention(**{switch: -1e30 if switch == "mask_value" else True})
    failed = []
    for case in sc.WIN_CASES:
        got = sc.as_got(sc.evaluate(case, attention=wrong))
        try:
            sc.check(case, got, E32[case.id])
        except AssertionError:
            failed.append(case.id)
    assert must_fail <= set(failed), (switch, sorted(must_fail - set(failed)))
    assert not unaffected & set(failed), (switch, sorted(unaffected & set(failed)))


def test_each_output_is_judged_on_its_own_and_per_block():
    """An error in dv alone, in one head of the masked corner window alone, fails dv and nothing else: the measure does not average."""
    case = WIN["win-f3-14x14-ws7-s3-h7"]
    got = sc.as_got(sc.reference(case))
    kw = case.kw
    rows = sc.blocks(torch.arange(3 * 196).view(3, 196, 1).expand(3, 196, 7 * 32).float(), kw)      # the token of every block element
    corner = rows.reshape(3, 4, 7, 49, 32)[2, 3, 6, :, 0].long()                                     # frame 2, window 3, head 6
    got["dv"].view(3 * 196, 7, 32)[corner, 6] *= 1 + 5e-5
    errs = {}
    for name in sc.WIN_OUTPUTS:
        errs[name] = sc.error(got[name], sc.reference(case)[name][1], kw)
    assert errs["dv"] > 2e-5 and max(errs[n] for n in ("out", "dq", "dk")) < 1e-7
    whole = float((got["dv"].double() - sc.reference(case)["dv"][1]).norm() / sc.reference(case)["dv"][1].norm())
    assert whole < 1e-5                                            # the relative L2 over the tensor, 1e-5 backward bound: blind to it
    with pytest.raises(AssertionError, match="dv error"):
        sc.check(case, got, E32[case.id])


def test_a_wrong_patch_merging_fails_the_table():
    def swapped(x, H, W):                                          # quarters 1 and 2 exchanged
        N, T, C = x.shape
        g = x.reshape(N, H, W, C)
        return torch.cat([g[:, 0::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 0::2], g[:, 1::2, 1::2]], -1).reshape(N, T // 4, 4 * C)
    for case in sc.MERGE_CASES:
        sc.check(case, sc.as_got(sc.evaluate(case)), {})
        with pytest.raises(AssertionError, match="merged differs"):
            sc.check(case, sc.as_got(sc.evaluate(case, gather=swapped)), {})
