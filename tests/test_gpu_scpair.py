"""The shortcut pair on the device (`k_conv_scpair`, csrc/i2v_conv_scpair.hip): a first bottleneck's projection shortcut and the expand
convolution that adds it as ONE launch -- backward, the shortcut's input gradient under conv1's -- against the same plan made with
I2V_SCPAIR=0, bit for bit, and against the oracle.  One-bottleneck nets at the smallest shapes at which the kernel can go wrong:

    stride 1   2 frames of 12 x 12, 64 -> 16 -> 80    288 pixels = 4.5 tiles (a pixel tail, a tile across two frames), channel tail 64 + 16
    K tail     the same with 24 input channels        K = 24 in a 32-row packing
    stride 2   3 frames of 16 x 16 -> 8 x 8, 48 -> 32 -> 128    the tap-uniform shortcut loop beside the pointwise expand loop, tiles exact
    7 x 7      a plane that is no multiple of 4       no dense epilogue: no pair, same results

Plans are made without the autotuner, so every admitted pair runs as one launch at every batch size."""
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from oracle import restate
from tests.test_gpu_parity import dev, write_hook_grads

pytestmark = pytest.mark.gpu

#        tag        frames plane stride cin mid cout  pairs (forward, backward)
CASES = [("stride1", 2, 12, 1, 64, 16, 80, (1, 1)),
         ("ktail", 2, 12, 1, 24, 16, 80, (1, 1)),
         ("stride2", 3, 16, 2, 48, 32, 128, (1, 0)),        # (the strided shortcut's gradient is a compact addend: it stays a launch)
         ("plane7", 2, 7, 1, 32, 16, 64, (0, 0))]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


def bottleneck_graph(plane, stride, cin, mid, cout):
    """input(3) -> 3x3 conv to `cin` channels -> ONE bottleneck with a projection shortcut, in torchvision's order of emission."""
    g = graphs.Graph("scpair_unit", (plane, plane))
    x = g.new_tensor(3, plane, plane, False, "input")
    g.input = x
    x = g.conv(x, cin, 3, 1, 1, "stem.weight", bias="stem.bias", relu=True, name="stem")
    a = g.conv(x, mid, 1, 1, 0, "b.conv1.weight", bn="b.bn1", name="b.conv1")
    a = g.conv(a, mid, 3, stride, 1, "b.conv2.weight", bn="b.bn2", name="b.conv2")
    idt = g.conv(x, cout, 1, stride, 0, "b.downsample.0.weight", bn="b.downsample.1", relu=False, name="b.downsample")
    y = g.conv(a, cout, 1, 1, 0, "b.conv3.weight", bn="b.bn3", residual=idt, name="b.out")
    g.hooks[1] = y
    return g, idt


def run(eng, g, sd, x, hg, planned, frames):
    """Plan for `planned` frames, run `frames`: (hooked feature, input gradient, pair info, pair launches)."""
    net = eng.build_net(g, sd, [g.hooks[1]], planned)
    info, s0 = net.scpair_info(), eng.capi.i2v_backend_stat(b"scpair_launches")
    net.forward(dev(x[:frames]))
    f = net.read_tensor(g.hooks[1], frames).cpu()
    write_hook_grads(net, [f], [hg[:frames]], frames)
    gx = torch.empty(frames, 3, x.shape[2], x.shape[3], device="cuda:0")
    net.backward(gx)
    torch.cuda.synchronize()
    out = f, gx.cpu(), info, eng.capi.i2v_backend_stat(b"scpair_launches") - s0
    net.close()
    return out


def both_plans(eng, monkeypatch, case, planned=None, frames=None):
    tag, n, plane, stride, cin, mid, cout, pairs = case
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    g, _ = bottleneck_graph(plane, stride, cin, mid, cout)
    sd = weights.synthetic_state_dict(g, 5)
    gen = torch.Generator().manual_seed(plane + cin)
    x = torch.randn(planned or n, 3, plane, plane, generator=gen)
    ho = g.tensors[g.hooks[1]].H
    hg = torch.randn(planned or n, cout, ho, ho, generator=gen)
    monkeypatch.delenv("I2V_SCPAIR", raising=False)
    fused = run(eng, g, sd, x, hg, planned or n, frames or n)
    monkeypatch.setenv("I2V_SCPAIR", "0")
    plain = run(eng, g, sd, x, hg, planned or n, frames or n)
    return g, sd, x, hg, fused, plain


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pair_is_bit_identical_to_the_two_launches(eng, monkeypatch, case):
    pairs = case[-1]
    _, _, _, _, fused, plain = both_plans(eng, monkeypatch, case)
    assert fused[2] == pairs + pairs and plain[2] == (0, 0, 0, 0), (fused[2], plain[2])
    assert fused[3] == sum(pairs) and plain[3] == 0                  # one launch per pair and pass; none without
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])
    assert bool(torch.isfinite(fused[0]).all()) and bool(torch.isfinite(fused[1]).all())


def test_pair_below_the_planned_batch(eng, monkeypatch):
    """Planned for 4 frames, run with 2: another batch bucket, another tile count (4.5 instead of 9 pixel tiles)."""
    _, _, _, _, fused, plain = both_plans(eng, monkeypatch, CASES[0], planned=4, frames=2)
    assert fused[3] == 2 and plain[3] == 0
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])


def test_pair_against_the_oracle_and_shortcut_read_back(eng, monkeypatch):
    """The stride-1 case against the float64 oracle at the tolerance of test_net_forward_backward_match_oracle; the shortcut's output,
    which the pair never stores, still reads back (produced on demand) with the bits the separate launch stores."""
    tag, n, plane, stride, cin, mid, cout, _ = CASES[0]
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    g, idt = bottleneck_graph(plane, stride, cin, mid, cout)
    sd = weights.synthetic_state_dict(g, 5)
    x = torch.randn(n, 3, plane, plane, generator=torch.Generator().manual_seed(3))
    onet = restate.OracleNet(g, sd, [g.hooks[1]], dtype=torch.float64)
    feats = onet.forward(x.double())
    hg = [torch.randn_like(f) for f in feats]
    shortcut = {}
    for off in (None, "0"):
        monkeypatch.delenv("I2V_SCPAIR", raising=False)
        if off:
            monkeypatch.setenv("I2V_SCPAIR", off)
        net = eng.build_net(g, sd, [g.hooks[1]], n)
        net.forward(dev(x))
        shortcut[off] = net.read_tensor(idt, n).cpu()
        if off is None:
            assert net.scpair_info() == (1, 1, 1, 1)
            got = net.read_tensor(g.hooks[1], n).cpu().double()
            assert (got - feats[0]).abs().max() <= 1e-4 * feats[0].abs().max() + 1e-6
            write_hook_grads(net, feats, hg, n)
            gx = torch.empty(n, 3, plane, plane, device="cuda:0")
            net.backward(gx)
            ref = onet.backward(hg)
            assert (gx.cpu().double() - ref).abs().max() / ref.abs().max() < 1e-4
        net.close()
    assert torch.equal(shortcut[None], shortcut["0"])
    assert (shortcut[None].double() - onet.tensor(idt)).abs().max() <= 1e-4 * onet.tensor(idt).abs().max() + 1e-6
