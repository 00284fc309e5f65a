"""Exact-size, guarded buffers for the workspace contract tests.

Every entry point that needs scratch takes ``(ws, ws_bytes)`` and has a ``*_workspace_bytes``
companion.  In normal use the Python side hands all of them one grow-only buffer
(``ops._workspace``: never below 1 MiB, rounded up by the caching allocator, as large as the
largest earlier request), so a kernel that writes past its own plan lands in slack and no output
check can see it.  Here every request gets a slice of EXACTLY the promised size with a guard of a
fixed non-zero byte on both sides; ``check()`` reads the guards back.

    arena = GuardedArena(dev)
    ws = arena.take(nbytes, label="csr_build ws")         # uint8 [nbytes], 256-byte aligned start
    out = arena.take(4 * (n + 1), torch.int32, (n + 1,))  # an output with nothing behind it
    ...launch...
    arena.check()                                         # synchronises, asserts on a dirty guard

``exact_workspaces(arena)`` swaps ``_workspace`` for an arena-backed allocator in ``ops`` and in
every module that bound the name at import, so the existing Python wrappers (and with them the
existing oracles) run unchanged against exact-size scratch.

What a kernel READS takes another byte: ``0xA5`` repeated is -2.87e-16 as f32 and bf16 and
-2.5e-127 as f64, which no sum, maximum or product notices, while ``0xFF`` repeated is NaN in
f32, f64, bf16 and f16 (and -1 in int32 / int64), and NaN x 0 is NaN: a stray read that is
"masked" by a zero multiplier or a zero softmax weight reaches the result, one that is dropped
by a select after the load does not.

    arena = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)   # NaN guards, NaN scratch
    x = arena.place(x)                        # same bits, last byte flush against the guard
    idx = arena.place(idx, guard_byte=0x00)   # a stray index reads 0: in range, wrong result
    with poisoned_fresh_tensors(dev), exact_workspaces(arena):
        ...                                   # torch.empty & co. hand out NaN on ``dev``

Works on CPU tensors too (tests/test_guarded_cpu.py checks the checker without a GPU).
"""
import contextlib
import functools
import importlib
import sys

import torch

GUARD_BYTE = 0xA5
ALIGN = 256

# modules that use ops._workspace; those that did `from .ops import _workspace` at import time
# hold a binding of their own, the rest import it inside their functions (then patching ops is
# enough, and patching them is a no-op)
WORKSPACE_USERS = ("ops", "segment", "neighbors", "graph", "transforms", "ground", "features",
                   "data", "csr", "instance")


class GuardError(AssertionError):
    pass


def _byte(b):
    b = int(b)
    if not 0 <= b <= 255:
        raise ValueError("a guard or fill byte is 0..255")
    return b


class GuardedArena:
    def __init__(self, dev, guard=1 << 20, guard_byte=GUARD_BYTE, fill_byte=None):
        if guard < 1 or guard % ALIGN:
            raise ValueError("guard must be a positive multiple of 256")
        self.dev = torch.device(dev)
        self.guard = int(guard)
        self.guard_byte = _byte(guard_byte)
        self.fill_byte = None if fill_byte is None else _byte(fill_byte)
        self._slices = []            # (label, backing uint8 tensor, start, nbytes)
        self._bytes = []             # the guard byte of each slice

    def take(self, nbytes, dtype=None, shape=None, label=None, guard_byte=None):
        """A view of exactly ``nbytes`` bytes between two guards: uint8 ``[nbytes]``, or with
        ``dtype`` / ``shape`` a tensor of that type and shape over the same bytes.  ``guard_byte``
        overrides the arena's for this slice; the contents are the arena's ``fill_byte``, or
        undefined when that is None."""
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError("negative size")
        g = self.guard
        gb = self.guard_byte if guard_byte is None else _byte(guard_byte)
        # over-allocate by one alignment unit: the view must START on a 256-byte boundary whatever
        # the allocator returns, and must not be rounded at its END
        back = torch.empty(g + nbytes + g + ALIGN, dtype=torch.uint8, device=self.dev)
        start = g + (-(back.data_ptr() + g)) % ALIGN
        back[:start].fill_(gb)
        back[start + nbytes:].fill_(gb)
        if self.fill_byte is not None:
            back[start:start + nbytes].fill_(self.fill_byte)
        if label is None:
            label = f"slice{len(self._slices)}"
        label = f"{label}[{nbytes} B]"
        self._slices.append((label, back, start, nbytes))
        self._bytes.append(gb)
        view = back[start:start + nbytes]
        assert view.data_ptr() % ALIGN == 0
        if dtype is None:
            return view
        t = view.view(dtype)
        if shape is not None:
            t = t.view(shape)
        return t

    def like(self, t, label=None):
        """An arena tensor of ``t``'s dtype and shape (contents undefined)."""
        return self.take(t.numel() * t.element_size(), t.dtype, tuple(t.shape), label)

    def place(self, t, guard_byte=None, label=None):
        """A copy of ``t`` (same dtype, shape and bits, contiguous) in a slice of exactly its size:
        it starts on a 256-byte boundary and its last byte lies against the guard, so a read one
        element past either end of it reads ``guard_byte``.  The result looks like a tensor its
        maker has just finished (``_version`` 0): the package memoises views on such tensors only."""
        out = self.take(t.numel() * t.element_size(), t.dtype, tuple(t.shape), label, guard_byte)
        out.copy_(t.detach())
        return out.data                     # the same bytes under a version counter of their own

    def __len__(self):
        return len(self._slices)

    def sizes(self):
        """The byte counts asked for so far, in order."""
        return [nbytes for _, _, _, nbytes in self._slices]

    def dirty(self):
        """[(label, side, first dirty offset, dirty byte count)].  ``side`` is "after" (offset
        counted from the END of the slice, 0 = the byte right behind it) or "before" (offset
        counted backwards from the start, 0 = the byte right in front of it)."""
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        found = []
        for (label, back, start, nbytes), gb in zip(self._slices, self._bytes):
            after = (back[start + nbytes:] != gb).nonzero().flatten()
            if after.numel():
                found.append((label, "after", int(after[0]), int(after.numel())))
            before = (back[:start].flip(0) != gb).nonzero().flatten()
            if before.numel():
                found.append((label, "before", int(before[0]), int(before.numel())))
        return found

    def check(self):
        found = self.dirty()
        if found:
            raise GuardError("; ".join(
                f"{label}: {cnt} guard byte(s) overwritten {side} the slice, first at offset {off} "
                f"{'past its end' if side == 'after' else 'before its start'}"
                for label, side, off, cnt in found))

    def release(self):
        self._slices.clear()
        self._bytes.clear()


def _modules():
    pkg = "superpoint_transformer_amd"
    mods = []
    for name in WORKSPACE_USERS:
        mods.append(importlib.import_module(f"{pkg}.{name}"))
    # anything else of the package already imported that holds the name
    for name, mod in list(sys.modules.items()):
        if name.startswith(pkg + ".") and mod is not None and mod not in mods \
                and "_workspace" in getattr(mod, "__dict__", {}):
            mods.append(mod)
    return mods


@contextlib.contextmanager
def exact_workspaces(arena):
    """Inside the block every ``_workspace(nbytes, dev)`` request of the package returns a fresh
    slice of exactly ``nbytes`` bytes of ``arena``; ``arena.check()`` runs on the way out (not
    when the block raised: the first error is the one to read)."""
    from superpoint_transformer_amd import ops
    real = ops._workspace

    def index_of(d):
        return d.index if d.index is not None or d.type != "cuda" else torch.cuda.current_device()

    def exact(nbytes, dev):
        dev = torch.device(dev)
        if dev.type != arena.dev.type:
            return real(nbytes, dev)                 # another kind of device: not this arena's business
        if index_of(dev) != index_of(arena.dev):
            raise GuardError(f"workspace asked on {dev} while the arena guards {arena.dev}: "
                             "nothing would be checked")
        return ops._handed_out(arena.take(nbytes, label=f"_workspace#{len(arena)}"))

    saved = []
    for mod in _modules():
        if "_workspace" in mod.__dict__:
            saved.append((mod, mod.__dict__["_workspace"]))
            mod._workspace = exact
    try:
        yield arena
    finally:
        for mod, old in saved:
            mod._workspace = old
    arena.check()


POISONED_FACTORIES = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"),
                      (torch.Tensor, "new_empty"))


@contextlib.contextmanager
def poisoned_fresh_tensors(dev):
    """Inside the block ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and
    ``Tensor.new_empty`` return NaN-filled tensors where the result is a floating-point tensor on
    ``dev``; integer tensors and other devices are left alone.  An element of an output or an
    intermediate that no kernel wrote then shows in whatever is computed from it.  The names are
    patched for every thread (autograd runs backward on its own) and restored on the way out."""
    dev = torch.device(dev)

    def on_dev(t):
        if t.device.type != dev.type:
            return False
        return dev.index is None or t.device.index is None or t.device.index == dev.index

    def poisoning(real):
        @functools.wraps(real)
        def fresh(*args, **kwargs):
            t = real(*args, **kwargs)
            if torch.is_tensor(t) and t.is_floating_point() and on_dev(t) and t.numel():
                t.detach().fill_(float("nan"))
            return t
        return fresh

    # (owner, name, the callable, whether the owner itself holds the name or inherits it)
    saved = [(owner, name, getattr(owner, name), name in vars(owner)) for owner, name in POISONED_FACTORIES]
    try:
        for owner, name, real, _ in saved:
            setattr(owner, name, poisoning(real))
        yield
    finally:
        for owner, name, real, own in saved:
            if own:
                setattr(owner, name, real)
            else:
                delattr(owner, name)
