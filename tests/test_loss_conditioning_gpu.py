"""The softmax criteria of csrc/loss.hip under confident, wide, shifted and masked logits, against
the float64 references and the derived bars of tests/loss_conditioning_cases.py (that the cases
tell a sound kernel from an unsound one is shown on the host by
tests/test_loss_conditioning_cpu.py).  Per route, kind, class count and both row counts:

* the loss and every gradient element within their bars, rows that do not count exactly 0, the
  entry at row 4's masked class exactly 0;
* a second call returns the same bits for the loss and the gradient;
* an upstream gradient of 2^-3 scales the gradient bit for bit.  An f32 below 2^-126 is
  subnormal and cannot hold the scaled value's last bits, so where |g| 2^-3 < 2^-126 the two may
  differ by the subnormal spacing 2^-149, and by nothing anywhere else;
* -inf at the target class of a counted row gives +inf, an all -inf row NaN, as float64 torch.

Every test prints its error / bar pairs (profiles/r26a_loss_conditioning_errors.txt)."""
import pytest
import torch

import loss_conditioning_cases as L

pytestmark = pytest.mark.gpu


def check(dev, route, kind, C, flag):
    measured = []
    for rows in L.ROWS:                                     # every figure out before any assertion
        c = L.case(route, kind, rows, C, 0, flag)
        loss, g = L.run(dev, c)
        gr, lr, zero_ok = L.ratios(c, loss, g)
        print(L.line(c, flag, gr, lr))
        measured.append((c, loss, g, gr, lr, zero_ok))
    for c, loss, g, gr, lr, zero_ok in measured:
        rows = c["rows"]
        assert bool(torch.isfinite(g).all())
        if bool(torch.isinf(c["loss"].float())):
            # 'huge' logits times class weights of 1e3 in histogram mode: the reference itself is
            # past the largest f32, and the f32 it rounds to is that infinity
            assert float(loss) == float(c["loss"].float())
        else:
            assert bool(torch.isfinite(loss))
            assert lr <= 1.0, (rows, lr)
        assert gr <= 1.0, (rows, gr)
        assert zero_ok
        if c["k4"] is not None:
            assert float(g[4, c["k4"]]) == 0.0
        loss2, g2 = L.run(dev, c)
        assert torch.equal(L.bits(loss2), L.bits(loss)) and torch.equal(L.bits(g2), L.bits(g))
        loss8, g8 = L.run(dev, c, gout=0.125)
        assert torch.equal(L.bits(loss8), L.bits(loss))
        normal = g.abs() * 0.125 >= 2.0 ** -126
        assert torch.equal(L.bits(g8[normal]), L.bits(g[normal] * 0.125))
        assert float((g8.double() - g.double() * 0.125).abs().max()) <= 2.0 ** -149


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("C", L.CLASSES)
@pytest.mark.parametrize("kind", L.KINDS)
def test_plain_cross_entropy(kind, C, ignore, dev):
    check(dev, "plain", kind, C, ignore)


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("C", L.CLASSES)
@pytest.mark.parametrize("kind", L.KINDS)
def test_weighted_index_cross_entropy(kind, C, ignore, dev):
    check(dev, "index", kind, C, ignore)


@pytest.mark.parametrize("void", [False, True])
@pytest.mark.parametrize("C", L.CLASSES)
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("mode", ["dominant", "histogram"])
def test_histogram_loss(mode, kind, C, void, dev):
    check(dev, mode, kind, C, void)


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("C", [c for c in L.CLASSES if c >= 2])
@pytest.mark.parametrize("mask", L.MASKS)
@pytest.mark.parametrize("route", L.ROUTES)
def test_masked_target_and_masked_row(route, mask, C, flag, dev):
    for kind in ("x3", "off-3e4"):
        c = L.case(route, kind, 257, C, 0, flag, mask)
        loss, g = L.run(dev, c)
        print(f"{route} {kind} C {C} flag {int(flag)} mask {mask}: loss {float(loss)} ref {float(c['loss'])}")
        assert (float(c["loss"]) == float("inf")) if mask == "target" else bool(torch.isnan(c["loss"]))
        assert L.same_kind(loss, c["loss"])
        # the other rows' gradients do not see row 0: those that do not count stay exactly 0
        assert bool((g[c["S"] == 0] == 0).all())
        loss2, g2 = L.run(dev, c)
        assert torch.equal(L.bits(loss2), L.bits(loss)) and torch.equal(L.bits(g2), L.bits(g))
