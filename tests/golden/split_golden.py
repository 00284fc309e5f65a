"""Store a fixture as parts that each stay below the repository's 1 MiB limit per file.

    python tests/golden/split_golden.py <name>.npz [...]

``<name>.npz`` -> ``<name>.part0.npz``, ``<name>.part1.npz``, ... (compressed), then the whole file
is removed.  An array too large for one part is cut along its first axis into ``<key>::<j>``
pieces; ``conftest.load_golden("<name>.npz")`` puts everything back together, bit for bit.
A file that is not an .npz (``<name>.<ext>``) is compressed with xz and cut into
``<name>.<ext>.xz.part<i>`` byte ranges (``conftest.golden_file`` reassembles it)."""
import io
import lzma
import os
import sys
import zipfile

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__))
LIMIT = 900 * 1024            # bytes per part (below 1 MiB with room for the zip directory)


def _compressed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def _pieces(key, a):
    """(name, array) pieces of one array, each small enough to compress below LIMIT alone."""
    n = _compressed_size({key: a})
    if n <= LIMIT or a.ndim == 0 or a.shape[0] < 2:
        return [(key, a)]
    k = -(-n // (LIMIT * 3 // 4))                 # aim at 3/4 of the limit per piece
    bounds = np.linspace(0, a.shape[0], k + 1).astype(int)
    return [(f"{key}::{j}", a[lo:hi]) for j, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:]))]


def split_npz(name):
    path = os.path.join(GOLDEN, name)
    stem = path[:-len(".npz")]
    with np.load(path) as d:
        items = [p for k in d.files for p in _pieces(k, d[k])]
    parts, cur = [], {}
    for k, a in items:
        if cur and _compressed_size({**cur, k: a}) > LIMIT:
            parts.append(cur)
            cur = {}
        cur[k] = a
    parts.append(cur)
    for i, p in enumerate(parts):
        np.savez_compressed(f"{stem}.part{i}.npz", **p)
        assert os.path.getsize(f"{stem}.part{i}.npz") < 1 << 20
    os.remove(path)
    return len(parts)


def split_bytes(src, name):
    data = lzma.compress(open(src, "rb").read(), preset=9 | lzma.PRESET_EXTREME)
    out = os.path.join(GOLDEN, name + ".xz")
    n = -(-len(data) // LIMIT)
    for i in range(n):
        with open(f"{out}.part{i}", "wb") as f:
            f.write(data[i * LIMIT:(i + 1) * LIMIT])
    return n


if __name__ == "__main__":
    for a in sys.argv[1:]:
        if a.endswith(".npz"):
            assert zipfile.is_zipfile(os.path.join(GOLDEN, a)), a
            print(a, split_npz(a), "parts")
        else:
            print(a, split_bytes(a, os.path.basename(a)), "parts")
