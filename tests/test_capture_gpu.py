"""The train step as a captured graph (hipGraph through torch.cuda.CUDAGraph, hotpath.SPTTrainStep.
capture): replays must be THE eager step - same losses, same parameter updates - for one cloud and
for a multi-cloud batch, with the optimizer inside the graph (one rank) and outside it (the flat
gradient bucket's collective path)."""
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _steps(dev, sizes, capture, n_steps=4, model="spt64", force_collective=False):
    from superpoint_transformer_amd import csr, hotpath
    from superpoint_transformer_amd.synthetic import make_nag
    nag = make_nag("R", seed=21, device=dev, sizes=sizes)
    path = hotpath.SPTTrainStep(nag, dev, seed=3, model=model)
    if force_collective:
        path.bucket.always = True
    losses = []
    if capture:
        path.capture(warmup=1)                # ONE eager step (the optimizer's state must exist), then capture
        assert path.graph is not None
        n_steps -= 1
    for _ in range(n_steps):
        losses.append(float(path.step().detach()))
    torch.cuda.synchronize()
    csr.verify_adopted(block=True)            # the captured check kernels' verdicts: nothing stale
    return losses, [p.detach().clone() for p in path.params]


def _far(pa, pb, n_steps, lr=1e-3):
    """Elements further apart than a fraction of one AdamW step (and none further than the steps
    taken)."""
    far = 0
    for a, b in zip(pa, pb):
        d = (a - b).abs()
        assert float(d.max()) <= 2.2 * n_steps * lr, float(d.max())
        far += int((d > 0.3 * lr).sum())
    return far


def _same_parameters(pe, pc, n_steps, pe2=None):
    """AdamW's first updates are lr * sign-like: a parameter whose gradient is rounding noise (the
    k-bias of every attention block - a softmax does not see a constant added to its keys - and
    every weight whose gradient nearly cancels; the backward's atomics reorder ~1e-6 of a tensor's
    scale between ANY two runs) walks +-lr per step in either run.  The yardstick is therefore a
    SECOND EAGER run (``pe2``): the captured run may differ from the eager one by what two eager
    runs differ by (x 2 + a sliver), not by a chosen fraction."""
    tot = sum(a.numel() for a in pe)
    far = _far(pe, pc, n_steps)
    base = _far(pe, pe2, n_steps) if pe2 is not None else 0.03 * tot
    print(f"parameters further apart than 0.3 lr: captured vs eager {far}, eager vs eager {base} of {tot}")
    # (two EAGER runs share their launch timing and with it most of the atomics' order - measured:
    # 0.14 % of the elements apart; a replayed graph has another timing, i.e. another sample of the
    # same rounding noise - measured: 1.1 %.  Noise-gradient elements only: the losses above agree.)
    assert far <= max(2 * base + 0.005 * tot, 0.03 * tot), (far, base, tot)


@pytest.mark.parametrize("sizes", [(30_000, 900, 380, 9_000, 7_000, 1), (40_000, 1_200, 500, 12_000, 9_000, 3)],
                         ids=["one-cloud", "three-clouds"])
def test_captured_step_is_the_eager_step(dev, sizes):
    """(Three runs of an atomics-noisy trajectory are compared: a fluke of the yardstick run - two
    eager runs that happen to agree unusually well - fails the comparison once in a few dozen
    visits.  The comparison is therefore repeated on fresh runs before it counts as a failure.)"""
    for attempt in range(3):
        try:
            _captured_vs_eager(dev, sizes)
            return
        except AssertionError:
            if attempt == 2:
                raise
            print(f"attempt {attempt + 1}: comparison outside its bound, repeating on fresh runs")


def _captured_vs_eager(dev, sizes):
    le, pe = _steps(dev, sizes, capture=False, n_steps=5)
    le2, pe2 = _steps(dev, sizes, capture=False, n_steps=5)
    lc, pc = _steps(dev, sizes, capture=True, n_steps=5)
    le, le2 = le[1:], le2[1:]                  # (the captured run's first step was its eager warm-up)
    # (the backward's dk / dv sums use hardware atomics: run-to-run differences of ~1e-6 of a
    # tensor's scale between ANY two runs, eager or not; AdamW's first steps are sign-like, so a
    # noise-gradient parameter walks +-lr per step and the losses of two runs drift apart by a few
    # 1e-4 within a handful of steps: the yardstick is a SECOND EAGER run)
    print("losses eager", le, "eager again", le2, "captured", lc)
    for a, a2, b in zip(le, le2, lc):
        assert abs(a - b) <= max(2e-4 * max(abs(a), 1.0), 4 * abs(a - a2)), (le, le2, lc)
    assert abs(le[0] - lc[0]) <= 2e-4 * max(abs(le[0]), 1.0)      # one update in: still tight
    assert le[-1] < le[0]                      # it trains
    _same_parameters(pe, pc, n_steps=5, pe2=pe2)


def test_captured_forward_backward_with_the_optimizer_outside(dev):
    """More than one rank: the graph ends after the backward, the flat all-reduce and AdamW run
    eagerly on the gradients the replay wrote.  Exercised here through the bucket's `always`
    switch without a process group (reduce() then only packs)."""
    from superpoint_transformer_amd import hotpath
    from superpoint_transformer_amd.synthetic import make_nag
    sizes = (30_000, 900, 380, 9_000, 7_000, 2)
    le, pe = _steps(dev, sizes, capture=False)
    nag = make_nag("R", seed=21, device=dev, sizes=sizes)
    path = hotpath.SPTTrainStep(nag, dev, seed=3)
    path.bucket.world = 2                      # as if a second rank existed: optimizer stays outside
    path.bucket.reduce = lambda: path.bucket.pack()
    path.capture(warmup=1)
    assert path.graph is not None and path._graph_opt is False
    lc = [float(path.step()) for _ in range(4)]
    # one warm-up step ran before the capture (fwd + bwd only: no update), so the replays start
    # from the same parameters as the eager run
    for k, (a, b) in enumerate(zip(le, lc)):
        # (first replay: the same parameters as the eager run's first step; later ones drift like
        # any two runs do - see test_captured_step_is_the_eager_step)
        assert abs(a - b) <= (2e-5 if k == 0 else 1.5e-3) * max(abs(a), 1.0), (le, lc)
    assert path.bucket.check_views()
    _same_parameters(pe, [p.detach() for p in path.params], n_steps=4)


# ---------------------------------------------------------------------------------------------------
# One deterministic comparison per test: everything below runs in the attention backward's SOURCE
# order (precision.attention_backward_order("source"): no float atomics), construction, capture and
# steps inside the block.  A run is then reproducible bit for bit, so a captured step can be held to
# the eager one without a yardstick run, a bound or a retry - a stale pointer in a replay, a skipped
# launch or scratch freed under the graph shows as a differing element.
# ---------------------------------------------------------------------------------------------------
ONE_CLOUD = (30_000, 900, 380, 9_000, 7_000, 1)
THREE_CLOUDS = (40_000, 1_200, 500, 12_000, 9_000, 3)
BOTH_SIZES = pytest.mark.parametrize("sizes", [ONE_CLOUD, THREE_CLOUDS], ids=["one-cloud", "three-clouds"])


def _path(dev, sizes, optimizer_outside=False):
    from superpoint_transformer_amd import hotpath
    from superpoint_transformer_amd.synthetic import make_nag
    nag = make_nag("R", seed=21, device=dev, sizes=sizes)
    path = hotpath.SPTTrainStep(nag, dev, seed=3)
    if optimizer_outside:                         # as if a second rank existed (reduce() only packs)
        path.bucket.world = 2
        path.bucket.reduce = lambda: path.bucket.pack()
    return path


def _finish(*paths):
    from superpoint_transformer_amd import csr
    torch.cuda.synchronize()
    csr.verify_adopted(block=True)
    return [[p.detach().clone() for p in path.params] for path in paths]


def _bitwise(what, names, got, want):
    """Prints the number of differing elements per tensor, then asserts that there is none."""
    bad = {}
    assert [t is None for t in got] == [t is None for t in want]      # (a parameter nothing reaches)
    names = [n for n, t in zip(names, got) if t is not None]
    got, want = [t for t in got if t is not None], [t for t in want if t is not None]
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        n = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        if n:
            bad[name] = (n, a.numel())
    print(f"{what}: {len(got)} tensors, {sum(t.numel() for t in got)} elements, differing per tensor: {bad or 0}")
    assert not bad and all(torch.equal(a, b) for a, b in zip(got, want)), f"{what} differ: {bad}"


def _copies(tensors):
    return [None if t is None else t.detach().clone() for t in tensors]


def _names(path):
    return [k for k, _ in path.model.named_parameters()]


@BOTH_SIZES
def test_eager_step_is_bitwise_reproducible(dev, sizes):
    """Two fresh steps of the same seed, 4 eager updates each: equal losses, equal parameters."""
    from superpoint_transformer_amd import precision
    with precision.attention_backward_order("source"):
        a, b = _path(dev, sizes), _path(dev, sizes)
        la = [float(a.step().detach()) for _ in range(4)]
        lb = [float(b.step().detach()) for _ in range(4)]
        pa, pb = _finish(a, b)
    print("losses", la, lb)
    assert la == lb
    _bitwise("parameters after 4 eager steps, run 1 vs run 2", _names(a), pa, pb)


def test_captured_gradients_are_the_eager_gradients(dev, sizes=ONE_CLOUD):
    """The optimizer outside the graph: the FIRST replay's gradients and loss are those of one eager
    forward + backward from the same initial parameters, bit for bit; after 3 more steps on both
    sides (AdamW eager on both) so are the parameters."""
    from superpoint_transformer_amd import precision
    with precision.attention_backward_order("source"):
        eager = _path(dev, sizes, optimizer_outside=True)
        le = float(eager.step().detach())                       # update 1 from the initial parameters
        ge = _copies(p.grad for p in eager.params)              # (AdamW leaves the gradients as they are)
        path = _path(dev, sizes, optimizer_outside=True)
        path.capture(warmup=1)                                  # warm-up: forward + backward only, no update
        assert path.graph is not None and path._graph_opt is False
        lc = float(path.step().detach())
        gc_ = _copies(path._graph_grads)
        _finish(eager, path)
        print("loss eager", le, "first replay", lc)
        assert le == lc
        _bitwise("gradients, first replay vs eager", _names(path), gc_, ge)
        for _ in range(3):
            eager.step()
            path.step()
        pe, pc = _finish(eager, path)
    assert path.bucket.check_views()
    _bitwise("parameters after 4 updates, replays vs eager", _names(path), pc, pe)


@BOTH_SIZES
def test_captured_step_with_the_optimizer_inside(dev, sizes):
    """One rank: AdamW inside the graph.  The eager twin runs the same AdamW arithmetic
    (``capturable=True`` in its param groups before its first step: the fused kernel with the step
    counter on the device, as the capture sets it); after the same number of updates - one eager
    warm-up update and 3 replays against 4 eager steps - the parameters are bitwise equal."""
    from superpoint_transformer_amd import precision
    with precision.attention_backward_order("source"):
        eager = _path(dev, sizes)
        for g in eager.opt.param_groups:
            g["capturable"] = True
        le = [float(eager.step().detach()) for _ in range(4)]
        path = _path(dev, sizes)
        path.capture(warmup=1)
        assert path.graph is not None and path._graph_opt is True
        lc = [float(path.step().detach()) for _ in range(3)]
        pe, pc = _finish(eager, path)
    print("losses eager", le, "captured", lc)
    assert le[1:] == lc
    _bitwise("parameters after 4 updates, optimizer in the graph vs eager", _names(path), pc, pe)


def test_replay_survives_cache_eviction_and_scratch_growth(dev):
    """A captured graph holds raw addresses of what ``ops._const_tensor`` and ``ops._workspace``
    handed out during warm-up and capture.  ``_CONST`` is cleared past 512 keys and a stream's
    scratch is replaced when a larger one is asked for: the step keeps every such tensor
    (``SPTTrainStep._graph_keep``), so neither frees memory that a replay reads.

    After one replay: 600 new constant tables, a larger scratch on a new stream and on every
    stream whose scratch the graph uses.  Then, ON THE HOST and before anything is replayed again:
    everything handed out during the capture is still held by the step, and none of its memory was
    given to a tensor created since.  Only then the second replay, whose gradients are those of an
    eager forward + backward from the same parameters, bit for bit."""
    from superpoint_transformer_amd import ops, precision
    with precision.attention_backward_order("source"):
        path = _path(dev, ONE_CLOUD, optimizer_outside=True)
        handed = []                                    # this test's own record of the two functions
        real_const, real_ws = ops._const_tensor, ops._workspace

        def spy(fn):
            def wrapped(*a, **k):
                t = fn(*a, **k)
                handed.append(t)
                return t
            return wrapped

        ops._const_tensor, ops._workspace = spy(real_const), spy(real_ws)
        try:
            path.capture(warmup=1)
        finally:
            ops._const_tensor, ops._workspace = real_const, real_ws
        path.graph.replay()                            # (no optimizer: the parameters stay the initial ones)
        torch.cuda.synchronize()

        kept = path._graph_keep
        assert handed and any(t.dtype != torch.uint8 for t in handed), "the capture took no constant table"
        assert all(any(t is k for k in kept) for t in handed), "a tensor handed out during the capture is not kept"
        spans = [(k.data_ptr(), k.data_ptr() + k.numel() * k.element_size()) for k in kept]

        created = [ops._const_tensor([1_000_003 + i, i], torch.int64, dev) for i in range(600)]
        assert len(ops._CONST) < 600                   # the cache was cleared on the way
        biggest = max(k.numel() for k in kept if k.dtype == torch.uint8)
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            created.append(ops._workspace(2 * biggest, dev))
        for (index, handle), buf in list(ops._WS.items()):
            if any(buf is k for k in kept):            # the capture's own stream: its scratch is replaced
                with torch.cuda.stream(torch.cuda.ExternalStream(handle, device=dev)):
                    created.append(ops._workspace(2 * buf.numel(), dev))
                assert ops._WS[(index, handle)] is not buf
        torch.cuda.synchronize()

        # the host-side verdict; nothing is replayed unless it holds
        assert path._graph_keep is kept and len(kept) == len(spans)
        assert [(k.data_ptr(), k.data_ptr() + k.numel() * k.element_size()) for k in kept] == spans
        for c in created:
            c0, c1 = c.data_ptr(), c.data_ptr() + c.numel() * c.element_size()
            assert not any(c0 < s1 and s0 < c1 for s0, s1 in spans), \
                "memory the graph reads was handed out again: not replaying"

        path.graph.replay()
        gc_ = _copies(path._graph_grads)
        lc = float(path._graph_loss.detach())
        eager = _path(dev, ONE_CLOUD, optimizer_outside=True)
        le = float(eager._fwd_bwd().detach())
        ge = _copies(p.grad for p in eager.params)
        _finish(eager, path)
    print("loss eager", le, "second replay", lc)
    assert le == lc
    _bitwise("gradients, replay after eviction vs eager", _names(path), gc_, ge)
