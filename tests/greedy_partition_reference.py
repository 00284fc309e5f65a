"""Host twin of the greedy contour-prior partition: numpy, f64, ``np.float32`` for the gains and
the weights.  Written from the specification of the rounds, not from the package's
code: plain loops, one group at a time.  The package has to agree with it label for label and
bit for bit, on the device and on the CPU.

Also the small graphs the tests share (``grid_case``).
"""
import numpy as np

LONG_RUN = 512
XOR_TREE = (32, 16, 8, 4, 2, 1)


# ---------------------------------------------------------------------------
# the two summation rules
# ---------------------------------------------------------------------------
def _op(reduce, a, b):
    if reduce == "max":
        return b if b > a else a
    if reduce == "min":
        return b if b < a else a
    if reduce == "mul":
        return a * b
    return a + b                                                   # add, mean


def reduce_weights(ws, reduce):
    """f32 reduction of the duplicates of one pair, in input order, from the first one."""
    ws = [np.float32(w) for w in ws]
    n = len(ws)
    if n <= LONG_RUN:
        acc = ws[0]
        for w in ws[1:]:
            acc = np.float32(_op(reduce, acc, w))
    else:
        part = []
        for lane in range(64):
            acc = ws[lane]
            for w in ws[lane + 64::64]:
                acc = np.float32(_op(reduce, acc, w))
            part.append(acc)
        for o in XOR_TREE:
            part = [np.float32(_op(reduce, part[l], part[l ^ o])) for l in range(64)]
        acc = part[0]
    if reduce == "mean":
        acc = np.float32(acc / np.float32(n))
    return acc


def sum_rows(rows):
    """f64 sum of the rows [n, c] in order, from 0."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[0]
    if n <= LONG_RUN:
        acc = np.zeros(rows.shape[1], dtype=np.float64)
        for r in rows:
            acc = acc + r
        return acc
    part = np.zeros((64, rows.shape[1]), dtype=np.float64)
    for lane in range(64):
        for r in rows[lane::64]:
            part[lane] = part[lane] + r
    for o in XOR_TREE:
        part = np.stack([part[l] + part[l ^ o] for l in range(64)])
    return part[0]


# ---------------------------------------------------------------------------
# graph
# ---------------------------------------------------------------------------
def component_graph(index, edge_index, edge_attr, reduce="add"):
    """``index`` None = identity.  Returns ([2, E'] int64 sorted by (lo, hi), [E'] f32)."""
    edge_index = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    E = edge_index.shape[1]
    w = np.ones(E, dtype=np.float32) if edge_attr is None else np.asarray(edge_attr, dtype=np.float32)
    groups = {}
    for e in range(E):                                             # input order
        a, b = int(edge_index[0, e]), int(edge_index[1, e])
        if index is not None:
            a, b = int(index[a]), int(index[b])
        if a == b:
            continue
        groups.setdefault((min(a, b), max(a, b)), []).append(w[e])
    keys = sorted(groups)
    out_e = np.array(keys, dtype=np.int64).reshape(-1, 2).T.copy()
    out_w = np.array([reduce_weights(groups[k], reduce) for k in keys], dtype=np.float32)
    return out_e, out_w


def edge_lengths(rows, edge_index):
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim == 1:
        rows = rows[:, None]
    out = np.zeros(edge_index.shape[1], dtype=np.float32)
    for e in range(edge_index.shape[1]):
        a, b = edge_index[0, e], edge_index[1, e]
        d2 = np.float64(0.0)
        for c in range(rows.shape[1]):
            t = np.float64(rows[a, c]) - np.float64(rows[b, c])
            d2 = d2 + t * t
        out[e] = np.float32(np.sqrt(d2))
    return out


def weights_from_lengths(dist, mode, d_0):
    """The elementwise part of the weight modes, f32; ``d_0`` an f32 scalar."""
    dist, d_0 = np.asarray(dist, dtype=np.float32), np.float32(d_0)
    if mode == "inverse_distance":
        return (np.float32(1) / (np.float32(1) + dist / d_0)).astype(np.float32)
    return np.exp(-(dist / d_0)).astype(np.float32)


# ---------------------------------------------------------------------------
# rounds
# ---------------------------------------------------------------------------
def gains(F, S, E, W, reg):
    out = np.zeros(E.shape[1], dtype=np.float32)
    m = F / S.astype(np.float64)[:, None]
    for e in range(E.shape[1]):
        a, b = E[0, e], E[1, e]
        d2 = np.float64(0.0)
        for d in range(F.shape[1]):
            t = m[a, d] - m[b, d]
            d2 = d2 + t * t
        sa, sb = np.float64(S[a]), np.float64(S[b])
        out[e] = np.float32(((sa * sb) / (sa + sb)) * d2 - np.float64(reg) * np.float64(W[e]))
    return out


def merge(X, S, E, W, reg, min_size, merge_only_small=False, max_iterations=-1, reduce="add",
          P=None, trace=None):
    """Returns (I, iterations, (X_merged f32, S int64, E_cp, W_cp f32, P_merged f32 or None)).
    ``trace``: a list that receives one dict per round (active count, jump passes, largest tree)."""
    X = np.asarray(X, dtype=np.float32)
    if X.ndim == 1:
        X = X[:, None]
    C = X.shape[0]
    S = np.asarray(S, dtype=np.int64).copy()
    F = X.astype(np.float64) * S.astype(np.float64)[:, None]
    Q = None if P is None else np.asarray(P, dtype=np.float32).astype(np.float64) * S.astype(np.float64)[:, None]
    E, W = component_graph(None, E, W, reduce)
    I = np.arange(C, dtype=np.int64)
    iterations = 0
    while E.shape[1] > 0 and not (0 < max_iterations <= iterations):
        C = S.shape[0]
        g = gains(F, S, E, W, reg)
        choice = {}                                                # a -> (g, b), least
        for e in range(E.shape[1]):
            a, b, ge = int(E[0, e]), int(E[1, e]), float(g[e])
            for u, v in ((a, b), (b, a)):
                if u not in choice or (ge, v) < choice[u]:
                    choice[u] = (ge, v)
        active = {a for a, (ga, _) in choice.items()
                  if S[a] < min_size or (not merge_only_small and ga < 0)}
        if not active:
            break
        parent = np.arange(C, dtype=np.int64)
        for a in active:
            parent[a] = choice[a][1]
        for a in active:
            b = choice[a][1]
            if b in active and choice[b][1] == a:
                parent[min(a, b)] = min(a, b)
        passes = 0
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent, passes = nxt, passes + 1
        roots = np.unique(parent)
        label = np.searchsorted(roots, parent)
        members = [[] for _ in roots]
        for old in range(C):                                       # ascending old id
            members[label[old]].append(old)
        S = np.array([sum(int(S[o]) for o in mem) for mem in members], dtype=np.int64)
        F = np.stack([sum_rows(F[mem]) for mem in members])
        if Q is not None:
            Q = np.stack([sum_rows(Q[mem]) for mem in members])
        E, W = component_graph(label, E, W, reduce)
        I = label[I]
        iterations += 1
        if trace is not None:
            trace.append(dict(active=len(active), passes=passes, largest=max(len(m) for m in members)))
    Sd = S.astype(np.float64)[:, None]
    X_merged = (F / Sd).astype(np.float32)
    P_merged = None if Q is None else (Q / Sd).astype(np.float32)
    return I, iterations, (X_merged, S, E, W, P_merged)


def merge_on_data(x, pos, edge_index, edge_attr, reg, min_size, super_index=None, node_size=None,
                  merge_only_small=False, max_iterations=-1, reduce="add"):
    """The level entry: nodes, or the components ``super_index``, merged.  Returns
    (super_index of every node, (X, S, E, W, P))."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[:, None]
    pos = np.asarray(pos, dtype=np.float32)
    N = x.shape[0]
    S = np.ones(N, dtype=np.int64) if node_size is None else np.asarray(node_size, dtype=np.int64)
    E, W = np.asarray(edge_index, dtype=np.int64), edge_attr
    if super_index is None:
        X_cp, P_cp, S_cp, I0 = x, pos, S, np.arange(N)
    else:
        I0 = np.asarray(super_index, dtype=np.int64)
        C0 = int(I0.max()) + 1
        members = [[] for _ in range(C0)]
        for i in range(N):
            members[I0[i]].append(i)
        Sd = S.astype(np.float64)[:, None]
        S_cp = np.array([sum(int(S[o]) for o in mem) for mem in members], dtype=np.int64)
        F = np.stack([sum_rows((x.astype(np.float64) * Sd)[mem]) for mem in members])
        Q = np.stack([sum_rows((pos.astype(np.float64) * Sd)[mem]) for mem in members])
        X_cp = (F / S_cp.astype(np.float64)[:, None]).astype(np.float32)
        P_cp = (Q / S_cp.astype(np.float64)[:, None]).astype(np.float32)
        E, W = component_graph(I0, E, W, reduce)
    I, it, out = merge(X_cp, S_cp, E, W, reg, min_size, merge_only_small, max_iterations, reduce, P_cp)
    return I[I0], it, out


# ---------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------
def grid_case(n, noise, D=2, seed=0):
    """An n x n grid: 8-neighbour edges listed in both directions, two feature columns forming
    four plateaus (+ seeded noise), ``D - 2`` further columns of noise at 0.01 (``D = 1`` keeps
    the first column only).  Returns (x [n*n, D] f32, pos [n*n, 3] f32, edge_index [2, E])."""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    cols = [(ii >= n // 2).astype(np.float64), (jj >= n // 2).astype(np.float64)]
    x = np.stack(cols, 1) + noise * rng.standard_normal((n * n, 2))
    if D > 2:
        x = np.concatenate([x, 0.01 * rng.standard_normal((n * n, D - 2))], 1)
    x = x[:, :D] if D < 2 else x
    pos = np.stack([ii, jj, 0.1 * rng.standard_normal(n * n)], 1)
    src, dst = [], []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di == 0 and dj == 0:
                continue
            ok = (ii + di >= 0) & (ii + di < n) & (jj + dj >= 0) & (jj + dj < n)
            src.append((ii * n + jj)[ok])
            dst.append(((ii + di) * n + jj + dj)[ok])
    edge_index = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    return x.astype(np.float32), pos.astype(np.float32), edge_index


def quotient(labels, edge_index, edge_attr, reduce="add"):
    """The input graph's quotient under final labels, computed directly."""
    return component_graph(np.asarray(labels), edge_index, edge_attr, reduce)


def bits(a):
    """A tensor or array as numpy, floats as their integer bits (NaN-safe, -0.0 != +0.0)."""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    if a.dtype == np.float32:
        return a.view(np.int32)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same(got, want):
    """(I, iterations, (X, S, E, W, P)) of the package == the twin's, bit for bit."""
    gI, git, (gX, gS, gE, gW, gP) = got
    wI, wit, (wX, wS, wE, wW, wP) = want
    assert git == wit, f"{git} rounds, the twin takes {wit}"
    for name, g, w in (("I_merged", gI, wI), ("S_merged", gS, wS), ("E_cp", gE, wE),
                       ("W_cp", gW, wW), ("X_merged", gX, wX)):
        g, w = bits(g), bits(w)
        assert g.shape == w.shape and np.array_equal(g, w), f"{name} differs from the twin"
    assert (gP is None) == (wP is None)
    if wP is not None:
        assert np.array_equal(bits(gP), bits(wP)), "P_merged differs from the twin"
