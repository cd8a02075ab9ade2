"""GPU (-m gpu): the 8-bit export and the quality launches on the MI355X (include/i2v_quality.h): every case of
tests/quality_cases.py on the device against float64 at the module's bounds, against the scalar host twin bit for bit, reruns bit for
bit, with the padding around `out` and `scratch` held; frame 0 of a 5-frame call against the 1-frame call; the launch counter and the
refusals, with the engine going on; `clip_to_u8` against its twin bit for bit, misaligned too; one `image_main.py --export_u8 --quality`
run on a tiny net with `reference.py` and `clip_quality.py` behind it."""
import pytest
import torch

from i2v_amd import attacks
from tests import quality_cases as qc
from tests.family_harness import stat
from tests.test_quality_cpu import FP32, check_cli_run, entry_refusals, twin_of, want_of

pytestmark = pytest.mark.gpu
COUNTER = b"quality_launches"


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _cuda(t):
    return t.cuda()


def _sync():
    torch.cuda.synchronize()


def test_the_case_table_brackets_the_tile(eng):
    assert eng.clip_quality_tile() == (qc.TR, qc.TC)


@pytest.mark.parametrize("case", qc.CASES, ids=lambda c: c.name)
def test_device_against_float64_and_the_host_twin(eng, case):
    a, b, want = want_of(case)
    s0 = stat(eng, COUNTER)
    got = qc.run_case(eng, case, a, b, _cuda, _sync)                  # (holds the padding of out and scratch)
    assert stat(eng, COUNTER) - s0 == 2                               # the tile launch and the frame launch
    n = want.shape[0]
    if case.reps > 1:
        assert torch.equal(got, got[:n].repeat(case.reps, 1))
    qc.check(case, got[:n], want, FP32)
    assert torch.equal(got, twin_of(case))                            # all three fields, the twin's bits
    assert torch.equal(got, qc.run_case(eng, case, a, b, _cuda, _sync))              # a rerun: the same bits
    if case.content == "same":
        assert torch.equal(got, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64).expand_as(got))


def test_frame_0_of_a_5_frame_call_has_the_bits_of_a_1_frame_call(eng):
    for name in ("u8-5x1x27x45-noise", "f32-2x3x27x45-noise"):
        case = qc.BY_NAME[name]
        a, b, _ = want_of(case)
        many = qc.run_case(eng, case, a, b, _cuda, _sync)
        one = qc.run_case(eng, case._replace(clips=1, t=1), a[:1, :, :1].contiguous() if case.mode == "f32" else a[:1],
                          b[:1, :, :1].contiguous() if case.mode == "f32" else b[:1], _cuda, _sync)
        assert torch.equal(many[:1], one)


def test_refusals_launch_nothing_and_the_engine_goes_on(eng):
    s0 = stat(eng, COUNTER)
    got = entry_refusals(eng, _cuda, _sync)
    assert stat(eng, COUNTER) - s0 == 2                               # only the call that follows the refusals
    assert torch.equal(got, twin_of(qc.BY_NAME["u8-1x1x27x13-noise"]))


def test_clip_to_u8_against_its_twin(eng):
    from tests.hostsim_util import hostsim_engine
    host = hostsim_engine()
    gen = torch.Generator().manual_seed(5)
    video = (torch.rand(2, 3, 3, 19, 23, generator=gen) * 6.0 - 3.0).contiguous()           # past both ends of [0, 1] after un-normalising
    video[0, 0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0])
    ref = torch.randint(0, 256, (2, 3, 19, 23, 3), generator=gen, dtype=torch.uint8)
    s0 = stat(eng, COUNTER)
    for kw in (dict(), dict(ref=ref, levels=12), dict(ref=ref, levels=12, offset=1), dict(ref=ref, levels=0), dict(offset=1)):
        assert torch.equal(qc.run_export(eng, video, to_dev=_cuda, sync=_sync, **kw), qc.run_export(host, video, **kw)), kw
    assert stat(eng, COUNTER) - s0 == 5
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16, 1).expand(1, 1, 16, 16, 3).contiguous().cuda()
    assert torch.equal(eng.clip_to_u8(eng.clip_from_u8(u8)), u8)                         # all 768 (level, channel) pairs come back


def test_image_main_with_both_flags_on_a_tiny_net(eng, tmp_path, monkeypatch):
    from i2v_amd import graphs
    monkeypatch.setenv("I2V_OPT_PATH", str(tmp_path))
    monkeypatch.setattr(graphs, "build", graphs.build_tiny)
    check_cli_run(eng, tmp_path, _cuda, same_bytes=False)
