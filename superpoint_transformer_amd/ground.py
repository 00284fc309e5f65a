"""Elevation above the ground (``GroundElevation``, src/transforms/point.py:185-326) on the
kernels of ``csrc/ground.hip``: the reference's three ground filters
(src/utils/ground.py:25-97), a RANSAC plane on the trimmed cloud (``single_plane_model``'s CPU
branch, ground.py:116-131) and the elevation of every point.

``ground_mask`` -> ``fit_ground_plane`` -> elevation; ``ground_elevation`` strings them together
and ``transforms.GroundElevation`` is a thin wrapper over it.

Host reads.  With ``xy_grid`` set, ``ground_mask`` reads five numbers back once (min z and the
extent of the cell coordinates) to size the dense cell table; ``fit_ground_plane`` /
``ground_elevation`` read back one eight-number status record at the end, to raise the
reference's errors.  Both are accepted: this is once-per-cloud preprocessing, not a captured
step.  The number of trimmed points never travels to the host in between.

Rules the reference leaves open, fixed here so that results are bitwise reproducible: among the
points of an XY cell that share the lowest z the lowest point index wins (``torch_scatter``'s
argmin does not say), and among hypotheses with equal inlier counts the lowest index wins."""
import torch

from . import _lib

__all__ = ["MAX_CELLS", "MAX_HYPOTHESES", "TrimmedCloud", "GroundPlane", "ground_mask",
           "fit_ground_plane", "plane_elevation", "ground_elevation"]

MAX_CELLS = 1 << 27          # dense cell table: 8 bytes per cell
MAX_HYPOTHESES = 256


class TrimmedCloud:
    """What ``ground_mask`` returns: ``index`` [capacity] int64, whose first ``count`` entries
    are the trimmed points in increasing point order, ``count`` [1] int64 ON THE DEVICE and
    ``num_points``.  ``indices()`` / ``mask()`` read the count back (a host sync): for callers
    outside the chain and for tests."""
    __slots__ = ("index", "count", "num_points")

    def __init__(self, index, count, num_points):
        self.index, self.count, self.num_points = index, count, int(num_points)

    def indices(self):
        return self.index[:int(self.count)]

    def mask(self):
        m = torch.zeros(self.num_points, dtype=torch.bool, device=self.index.device)
        m[self.indices()] = True
        return m


class GroundPlane:
    """The fit's record.  ``status`` [8] f64 and ``counts`` [H] int32 stay on the device;
    ``read()`` brings the status back once and fills ``num_trimmed`` (M), ``best_count``,
    ``best_index``, ``a``, ``b``, ``c`` (z = a x + b y + c), ``num_valid`` (hypotheses that
    were not degenerate) and ``num_refit`` (inliers of the final least-squares fit; -1 when they
    were rank-deficient and the plane is the best hypothesis's own)."""
    __slots__ = ("status", "counts", "num_trimmed", "best_count", "best_index", "a", "b", "c",
                 "num_valid", "num_refit")

    def __init__(self, status, counts):
        self.status, self.counts = status, counts
        self.num_trimmed = None

    def read(self):
        if self.num_trimmed is None:
            s = self.status.tolist()                                # host sync
            self.num_trimmed, self.best_count, self.best_index = int(s[0]), int(s[1]), int(s[2])
            self.a, self.b, self.c = s[3], s[4], s[5]
            self.num_valid, self.num_refit = int(s[6]), int(s[7])
        return self

    def check(self):
        """The reference's errors: sklearn's RANSAC raises on fewer samples than a plane needs
        and when no trial produced a valid model."""
        self.read()
        if self.num_trimmed < 3:
            raise ValueError(f"the ground filters left {self.num_trimmed} points: a plane needs 3")
        if self.num_valid == 0 or self.best_index < 0:
            raise ValueError("RANSAC found no valid hypothesis: every triplet repeated a point "
                             "or was degenerate in XY")
        return self

    @property
    def plane(self):
        self.read()
        return self.a, self.b, self.c


def _pos(pos):
    _lib.require_cuda(pos)
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must be [N, 3], got {tuple(pos.shape)}")
    n = pos.shape[0]
    if n >= 1 << 31:
        raise ValueError("more than 2^31 - 1 points")
    return pos.detach().float().contiguous()


def ground_mask(pos, z_threshold=None, verticality=None, verticality_threshold=None, xy_grid=None,
                max_cells=MAX_CELLS):
    """The trimmed cloud of ``GroundElevation._process`` (point.py:279-303): the points with
    ``z - z.min() < z_threshold`` and ``verticality < verticality_threshold`` that are the lowest
    of their ``xy_grid`` cell; each term applies only when its parameter is set.  The cell filter
    runs over ALL points like the reference's, with the cell ``trunc(x / grid)``,
    ``trunc(y / grid)`` of ``xy_partition``.

    The cells live in a dense table of (extent in i) x (extent in j) 64-bit keys; more than
    ``max_cells`` of them raise ``ValueError`` (one far outlier is enough).  Returns a
    ``TrimmedCloud``."""
    from .ops import _workspace
    posf = _pos(pos)
    n = posf.shape[0]
    dev = posf.device
    if n == 0:
        raise ValueError("the cloud is empty")
    vert = None
    if verticality_threshold is not None:
        if verticality is None:
            raise ValueError("verticality_threshold needs the verticality")
        _lib.require_cuda(verticality)
        vert = verticality.detach().float().reshape(-1).contiguous()
        if vert.numel() != n:
            raise ValueError("verticality must hold one value per point")
    L = _lib.lib
    stream = _lib.stream_ptr(dev)
    grid = float(xy_grid) if xy_grid else 0.0
    use_z = z_threshold is not None

    bounds = table = None
    cells = 0
    if use_z or grid > 0:
        bounds = torch.empty(8, dtype=torch.float32, device=dev)
        nbytes = L.spt_ground_bounds_workspace_bytes(n)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            st = L.spt_ground_bounds_f32(_lib.ptr(posf), n, grid, _lib.ptr(bounds), _lib.ptr(ws),
                                         ws.numel(), stream)
        _lib.check(st, "spt_ground_bounds_f32")
    if grid > 0:
        b = bounds[:5].tolist()                                     # host sync: sizes the table
        if not all(v == v and abs(v) != float("inf") for v in b[1:]):
            raise ValueError("pos holds non-finite x / y coordinates")
        i_min, i_max, j_min, j_max = (int(v) for v in b[1:])
        ni, nj = i_max - i_min + 1, j_max - j_min + 1
        cells = ni * nj
        if cells > max_cells:
            raise ValueError(
                f"xy_grid = {grid:g} over the cloud's extent needs a table of {ni} x {nj} = {cells} "
                f"cells (x cells {i_min}..{i_max}, y cells {j_min}..{j_max}), above the cap of "
                f"{max_cells}: a far outlier is the likely cause")
        table = torch.empty(cells, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            st = L.spt_ground_cell_min_f32(_lib.ptr(posf), n, grid, i_min, j_min, ni, nj,
                                           _lib.ptr(table), stream)
        _lib.check(st, "spt_ground_cell_min_f32")

    capacity = min(n, cells) if table is not None else n
    index = torch.empty(capacity, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = L.spt_ground_trim_workspace_bytes(n)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_ground_trim_f32(_lib.ptr(posf), n, _lib.ptr(bounds), int(use_z),
                                   float(z_threshold) if use_z else 0.0, _lib.ptr(vert),
                                   float(verticality_threshold) if vert is not None else 0.0,
                                   _lib.ptr(table), cells, _lib.ptr(index), capacity,
                                   _lib.ptr(count), _lib.ptr(ws), ws.numel(), stream)
    _lib.check(st, "spt_ground_trim_f32")
    return TrimmedCloud(index, count, n)


def fit_ground_plane(pos, trimmed, num_hypotheses=100, residual_threshold=1e-3, seed=0,
                     samples=None, check=True):
    """RANSAC plane ``z = a x + b y + c`` of the trimmed cloud with the vertical residual
    ``|z - z_hat| < residual_threshold`` (``RANSACRegressor(residual_threshold)`` on (xy, z),
    ground.py:121-124), then the least-squares fit on the best hypothesis's inliers (sklearn's
    final ``LinearRegression``), in f64.

    The ``num_hypotheses`` (default 100 = the reference's ``max_trials``) triplets come from
    ``torch.rand(H, 3)`` of a device generator seeded with ``seed``, mapped to
    ``min(floor(u M), M - 1)`` by the kernel, which reads M itself; ``samples`` [H, 3] int64
    (positions in the trimmed set) fixes them instead.  All hypotheses are scored in one pass
    over the trimmed points; there is no early stop, so the draw does not depend on the data.

    Returns a ``GroundPlane``; with ``check`` its status is read back and ``ValueError`` raised
    when fewer than 3 points were left or no hypothesis was valid."""
    from .ops import _workspace
    posf = _pos(pos)
    n = posf.shape[0]
    dev = posf.device
    if n == 0:
        raise ValueError("the cloud is empty")
    _lib.require_cuda(trimmed.index, trimmed.count)
    L = _lib.lib
    u = None
    if samples is not None:
        _lib.require_cuda(samples)
        samples = samples.long().contiguous()
        if samples.dim() != 2 or samples.shape[1] != 3:
            raise ValueError("samples must be [H, 3]")
        H = samples.shape[0]
    else:
        H = int(num_hypotheses)
    if not 1 <= H <= MAX_HYPOTHESES:
        raise ValueError(f"the number of hypotheses must be in [1, {MAX_HYPOTHESES}], got {H}")
    if samples is None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        u = torch.rand(H, 3, generator=gen, device=dev, dtype=torch.float32)
    counts = torch.empty(H, dtype=torch.int32, device=dev)
    status = torch.empty(8, dtype=torch.float64, device=dev)
    index = trimmed.index.contiguous()
    nbytes = L.spt_ground_ransac_workspace_bytes(H)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_ground_ransac_f32(_lib.ptr(posf), n, _lib.ptr(index), _lib.ptr(trimmed.count),
                                     max(index.numel(), 1), _lib.ptr(u), _lib.ptr(samples), H,
                                     float(residual_threshold), _lib.ptr(counts), _lib.ptr(status),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(st, "spt_ground_ransac_f32")
    plane = GroundPlane(status, counts)
    return plane.check() if check else plane


def plane_elevation(pos, plane, scale=1.0):
    """``(z - (a x + b y + c)) / scale`` [N, 1] f32 with the plane read on the device."""
    posf = _pos(pos)
    n = posf.shape[0]
    dev = posf.device
    out = torch.empty((n, 1), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        st = _lib.lib.spt_ground_elevation_f32(_lib.ptr(posf), n, _lib.ptr(plane.status),
                                               float(scale), _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(st, "spt_ground_elevation_f32")
    return out


def ground_elevation(pos, z_threshold=None, verticality=None, verticality_threshold=None,
                     xy_grid=None, scale=3.0, num_hypotheses=100, residual_threshold=1e-3,
                     random_state=0, samples=None, max_cells=MAX_CELLS):
    """``GroundElevation._process`` with ``model='ransac'`` (point.py:268-326): filters, plane,
    elevation / ``scale``.  Returns ``(elevation [N, 1] f32, GroundPlane)``; the plane's status
    has been read back (one host sync, after the elevation kernel was queued) and checked."""
    if not scale > 0:
        raise ValueError("scale must be positive")
    trimmed = ground_mask(pos, z_threshold, verticality, verticality_threshold, xy_grid,
                          max_cells=max_cells)
    plane = fit_ground_plane(pos, trimmed, num_hypotheses, residual_threshold, random_state,
                             samples=samples, check=False)
    elevation = plane_elevation(pos, plane, scale)
    plane.check()
    return elevation, plane
