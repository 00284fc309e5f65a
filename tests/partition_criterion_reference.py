"""Host twin of csrc/partition_loss.hip in numpy float64: the node labels, the edge classes, the
adaptive sample (``rand32`` of tests/augment_reference.py, the generator of csrc/rng.hpp) and the
loss with its gradient, every rule restated without looking at the kernels' order of evaluation.

Decisions (labels, classes, counters, the selected mask) are integers and compare exactly; the
loss and the gradient are float64 sums in plain edge order - the yardstick of the precision tests.
"""
import numpy as np

from augment_reference import rand32

CLAMPED = 1
_M64 = (1 << 64) - 1


def node_labels(y, num_classes):
    """int64 [N]: the first maximum of the class columns, -1 for a void node (maximum 0); a 1-D
    ``y`` holds labels, anything outside [0, num_classes) is void."""
    y = np.asarray(y).astype(np.int64)
    c = int(num_classes)
    if y.ndim == 1:
        return np.where((y >= 0) & (y < c), y, -1)
    best = y[:, :c].max(axis=1)
    label = y[:, :c].argmax(axis=1)                # numpy: the first maximum
    return np.where(best == 0, -1, label).astype(np.int64)


def classify(y, edge_index, num_classes):
    """``(code, bad)``: code uint8 [E] = 0 dropped / 1 inter / 2 intra, bad = edges with an end
    outside [0, N)."""
    label = node_labels(y, num_classes)
    n = label.shape[0]
    i, j = (np.asarray(edge_index[k]).astype(np.int64) for k in (0, 1))
    ok = (i >= 0) & (i < n) & (j >= 0) & (j < n)
    li, lj = label[np.clip(i, 0, n - 1)], label[np.clip(j, 0, n - 1)]
    kept = ok & (i != j) & (li >= 0) & (lj >= 0)
    code = np.where(kept, np.where(li == lj, 2, 1), 0).astype(np.uint8)
    return code, int((~ok).sum())


def call_seed(seed, calls):
    """The stream of call number ``calls``: seed ^ (rand32(0x5EED, 2 calls) << 32 | rand32(0x5EED,
    2 calls + 1))."""
    hi, lo = (int(v) for v in rand32(0x5EED, np.array([2 * calls, 2 * calls + 1], dtype=np.uint64)))
    return ((int(seed) & _M64) ^ ((hi << 32) | lo)) & _M64


def major_count(n_inter, ratio):
    """torch's ``((1 / ratio - 1) * count).int()``: one f32 product, truncated."""
    return int(np.float32(n_inter) * np.float32(1.0 / ratio - 1.0))


def select(code, ratio=None, state=(0, 0)):
    """``(selected bool [E], n_major, clamped)``; every inter edge, and the ``n_major`` intra edges
    with the smallest (draw, position) pairs."""
    inter, intra = code == 1, code == 2
    n_inter, n_intra = int(inter.sum()), int(intra.sum())
    if ratio is None:
        return inter | intra, n_intra, 0
    n_major, clamped = max(major_count(n_inter, ratio), 0), 0
    if n_major > n_intra:
        n_major, clamped = n_intra, CLAMPED
    pos = np.nonzero(intra)[0]
    draw = rand32(call_seed(*state), pos.astype(np.uint64))
    order = np.lexsort((pos, draw))                # by draw, ties by position
    sel = inter.copy()
    sel[pos[order[:n_major]]] = True
    return sel, n_major, clamped


def edge_terms(x, edge_index, selected, code, temperature, gamma, weight, epsilon):
    """Per selected edge, float64: ``(e, d, l, c)`` with c = dl/dd / d (0 at d == 0)."""
    x = np.asarray(x, dtype=np.float64)
    e = np.nonzero(selected)[0]
    i, j = np.asarray(edge_index[0])[e], np.asarray(edge_index[1])[e]
    t = code[e] == 2
    d = np.sqrt(((x[i] - x[j]) ** 2).sum(axis=1))
    p = np.exp(-d / temperature)
    q = np.where(t, p, 1 - p)
    qp = epsilon + (1 - 2 * epsilon) * q
    w = np.where(t, weight, 1 - weight)
    if gamma == 0:
        l = -w * np.log(qp)
        dl = -w / qp
    else:
        l = -w * (1 - qp) ** gamma * np.log(qp)
        dl = w * (gamma * (1 - qp) ** (gamma - 1) * np.log(qp) - (1 - qp) ** gamma / qp)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = dl * (1 - 2 * epsilon) * np.where(t, 1.0, -1.0) * (-p / temperature) / d
    c = np.where(d > 0, c, 0.0)
    return e, d, l, c


def loss_and_grad(x, y, edge_index, num_classes, temperature=1.0, gamma=0.0, weight=0.5,
                  epsilon=1e-6, ratio=None, state=(0, 0)):
    """Everything one call computes: ``loss`` (f64), ``grad`` f64 [N, D] for an upstream gradient
    of 1, ``counts`` (n_inter, n_intra, n_selected), ``selected``, ``code``, ``bad``, ``clamped``."""
    x = np.asarray(x, dtype=np.float64)
    code, bad = classify(y, edge_index, num_classes)
    sel, n_major, clamped = select(code, ratio, state)
    n_inter, n_intra = int((code == 1).sum()), int((code == 2).sum())
    n_sel = n_inter + n_major
    assert n_sel == int(sel.sum())
    out = dict(counts=(n_inter, n_intra, n_sel), selected=sel, code=code, bad=bad, clamped=clamped)
    grad = np.zeros_like(x)
    if n_inter == 0 or n_sel == 0:                  # the reference's fake loss
        out.update(loss=0.0, grad=grad)
        return out
    e, d, l, c = edge_terms(x, edge_index, sel, code, temperature, gamma, weight, epsilon)
    i, j = np.asarray(edge_index[0])[e], np.asarray(edge_index[1])[e]
    diff = c[:, None] * (x[i] - x[j])
    np.add.at(grad, i, diff)
    np.add.at(grad, j, -diff)
    out.update(loss=float(l.sum() / n_sel), grad=grad / n_sel)
    return out
