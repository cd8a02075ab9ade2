"""GPU (-m gpu): the window-attention and patch-merging case table (tests/swin_cases.py) through the C entries on the gfx950 kernels of
csrc/i2v_swin.hip -- swin_window_attention(_bwd), which every Swin block and every Twins-SVT window block runs on, and
swin_merge_gather / swin_merge_scatter, which Swin, ConvNeXt and Twins run on.  Per case:

  * the device against the reference, every output at its bound (swin_cases.check: out, dq, dk and dv each on its own, the error
    taken per (frame, window, head) block and held to max(2e-6, 4 e32), e32 from tests/golden/swin_kernel_fp32_cpu_errors.json;
    patch merging and the slack around every output bit for bit);
  * a second run of the same case gives the same bits.

Frame 0 of an n-frame call has the bits of a 1-frame call; a table pointer 4 bytes off 16-byte alignment changes no bit; the Twins
entries on the zero-table case are the Swin entries bit for bit; the merge grid's second trip is crossed by 136 quads; every refusal
names its launch and launches nothing, and an ordinary case runs after them.

Measured on an MI355X: 27 tests in 3.5 s; the slowest is the first case (0.93 s: it opens the engine), then the merge past the
cap (0.18 s) and the 3-frame, 7-head case (0.05 s); every other test takes <= 0.02 s.  Worst device error per output, measured as its
bound is, next to the bound it was held to and the e32 behind it -- over the 13 ordinary cases, and for each `hot` case:

    cases     output  error     bound     e32       case
    ordinary  out     6.72e-07  2.53e-06  6.33e-07  win-f2-21x14-ws7-s1-h2
    ordinary  dq      1.24e-06  4.16e-06  1.04e-06  win-f3-14x14-ws7-s3-h7
    ordinary  dk      1.38e-06  2.84e-06  7.09e-07  win-f1-21x14-ws7-s6-h3
    ordinary  dv      6.61e-07  2.18e-06  5.44e-07  win-f1-21x14-ws7-s6-h3
    hot ws 7  out     1.04e-05  3.02e-05  7.55e-06  win-f1-14x14-ws7-s3-h2-hot
    hot ws 7  dq      5.40e-05  1.34e-04  3.34e-05
    hot ws 7  dk      5.55e-05  1.35e-04  3.37e-05
    hot ws 7  dv      4.95e-06  1.45e-05  3.63e-06
    hot ws 4  out     9.04e-06  5.00e-05  1.25e-05  win-f1-8x8-ws4-s2-h5-hot
    hot ws 4  dq      0.395     1.58      0.395
    hot ws 4  dk      0.551     2.2       0.551
    hot ws 4  dv      8.29e-06  2.67e-05  6.68e-06

No device error exceeds 0.49 of its bound, every exact output and every sentinel came back bit for bit, and all 49 refusals were
made: the table found no fault in the kernels.  One pair of bounds says nothing: dq and dk of the window-4 `hot` case.  At 16 keys and
logits of +-144 whole blocks have a one-hot softmax in every row, so their dq and dk are the rounding residue of dP - rowsum(dP P):
the worst block's largest |dq| is 8e-5 where the tensor's is 431, float32 torch is off by 0.4 of THAT, and the per-block measure
takes it for the case's error.  That case is there for out and dv (the -100 semantics); dq and dk under heat are held by the window-7
`hot` case, whose worst block has max|dq| = 15.  The errors are printed (pytest -s).
"""
import pytest
import torch

from i2v_amd import attacks
from tests import swin_cases as sc
from tests.make_swin_kernel_fixtures import load

pytestmark = pytest.mark.gpu

E32 = load()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


def _same(a, b):
    assert a.keys() == b.keys()
    return [n for n in a if not sc.same_bits(a[n], b[n])]


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_swin_case_on_the_device(eng, case):
    first = sc.run(eng, case)
    second = sc.run(eng, case)
    errs = sc.check(case, first, E32.get(case.id, {}), report=print)
    diff = _same(first, second)
    assert not diff, f"{case.id}: a second run changed {diff}"
    assert errs is not None


@pytest.mark.parametrize("cid", sc.FRAME_INVARIANCE)
def test_frame_0_has_the_bits_of_a_one_frame_call(eng, cid):
    case = sc.BY_ID[cid]
    whole, alone = sc.run(eng, case), sc.run(eng, case, frames=1)
    for name in sc.WIN_OUTPUTS:
        assert alone[name].shape[0] == 1 and sc.same_bits(alone[name][0], whole[name][0]), (cid, name)
    assert bool((alone["out_slack"] == sc.SENTINEL).all()) and bool((alone["dqkv_slack"] == sc.SENTINEL).all())


@pytest.mark.parametrize("cid", ("win-f3-14x14-ws7-s3-h7", "win-f1-8x12-ws4-s1-h3"))
def test_an_unaligned_table_changes_no_bit(eng, cid):
    case = sc.BY_ID[cid]
    diff = _same(sc.run(eng, case), sc.run(eng, case, table_off=1))
    assert not diff, (cid, diff)


def test_the_twins_entries_are_the_swin_entries_bit_for_bit(eng):
    case = sc.BY_ID[sc.NOTABLE]
    twins = sc.run(eng, case, route="twins")
    sc.check(case, twins, E32[case.id])
    diff = _same(sc.run(eng, case), twins)
    assert not diff, diff


def test_merging_past_the_grid_cap(eng):
    """(1, 2, 4, 8388676): 16 777 352 quads, 136 past the 65536 x 256 one trip of the grid covers.  Element i holds the int32 i, the
    gather is compared with the reference's permutation of the same integers and the scatter (accumulate 0) must undo it; int32
    compares on the device, slack included.  Measured on an MI355X: the two launches take 0.3 ms (1.07 GB moved), the test 0.18 s with its
    allocations and compares: both halves are kept."""
    bad, seconds = sc.run_merge_big(eng)
    print(f"merge past the cap: launches {seconds * 1e3:.1f} ms, mismatches {bad}")
    assert not any(bad.values()), bad


def test_refusals_name_their_launch_and_the_engine_goes_on(eng):
    thunks, untouched, keep = sc.refusals(eng)
    assert len(thunks) >= 40
    for label, name, thunk in thunks:
        assert thunk() != 0, (name, label)
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ":"), (label, text)
    assert untouched()
    del keep
    for cid in ("win-f1-14x21-ws7-s3-h1", "merge-f3-6x4-C20"):
        sc.check(sc.BY_ID[cid], sc.run(eng, sc.BY_ID[cid]), E32.get(cid, {}))
