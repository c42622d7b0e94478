"""Poisoned scratch and guarded buffers: does a result depend on what the workspace or the output held before the call?

The library clears next to nothing of the workspace it is handed; an array of it is right only because every element is
written before it is read, on every route.  A fresh process gets zero pages from the driver, so a read of never-written
scratch shows as a failure that moves with the order of the tests, or not at all.  The helpers here make it
deterministic:

guarded(nbytes, fill, device)   one uint8 allocation of GUARD + nbytes + GUARD bytes, both guard bands GUARD_BYTE, the
                                interior `fill`; workspaces and outputs are interiors, so a kernel that writes past the
                                last carved array (the carve functions check no bounds) lands in memory the test owns
                                and is counted by guards_intact(), and no access of the harness leaves an allocation.
PATTERNS                        what the interior of a workspace holds when the call under test begins, from the least
                                to the most hostile: zeros, the leavings of a call of the same entry point on the same
                                shape and parameters on other inputs (plausible floats, counts and flags at the very
                                offsets the call will use), and 0xFF (NaN floats, -1 ints, set flags, all-ones counts).
first_difference(run, differs)  runs the patterns in that order and stops at the first whose result differs: a more
                                hostile pattern is not run after a failure.

GUARD is one 64-row tile of 4096 float32 columns, the largest unit any kernel of the library writes at once (a condition,
not a measurement), and a multiple of 256, so an interior keeps the 256-byte alignment tri_sum_threshold_flagger demands
of its workspace and the 16-byte alignment its vector kernels want of an output.
"""
import numpy as np

GUARD = 1 << 20
GUARD_BYTE = 0xA5
OUTPUT_FILL = 0xEE
PATTERNS = ("zeros", "stale", "ones")
FILL = {"zeros": 0x00, "stale": 0x00, "ones": 0xFF}     # ("stale": the fill before the priming call overwrites it)

assert GUARD % 256 == 0 and GUARD == 64 * 4096 * 4


def guarded(nbytes, fill, device):
    """``(interior, whole)``: ``whole`` is one uint8 tensor of GUARD + nbytes + GUARD bytes on ``device`` whose guard bands
    hold GUARD_BYTE, ``interior`` the view of its middle ``nbytes`` bytes, filled with ``fill``."""
    import torch
    nbytes = int(nbytes)
    assert nbytes >= 0 and 0 <= int(fill) <= 0xFF
    whole = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)
    interior = whole[GUARD:GUARD + nbytes]
    interior.fill_(int(fill))
    assert nbytes == 0 or interior.data_ptr() - whole.data_ptr() == GUARD
    if whole.is_cuda and nbytes:
        assert interior.data_ptr() % 256 == 0
    return interior, whole


def guards_intact(whole, nbytes):
    """The number of guard bytes of ``guarded(nbytes, ...)[1]`` that no longer hold GUARD_BYTE (0: intact)."""
    nbytes = int(nbytes)
    assert whole.numel() == GUARD + nbytes + GUARD
    return int((whole[:GUARD] != GUARD_BYTE).sum()) + int((whole[GUARD + nbytes:] != GUARD_BYTE).sum())


class Output:
    """An output buffer of ``shape`` and torch ``dtype``: the interior of a guarded tensor, pre-filled with OUTPUT_FILL
    (``fill`` another byte, or a host array whose values the call is to continue from)."""

    def __init__(self, shape, dtype, device, fill=OUTPUT_FILL):
        import torch
        self.shape = tuple(int(s) for s in shape)
        n = int(np.prod(self.shape, dtype=np.int64))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        raw, self.whole = guarded(self.nbytes, fill if np.isscalar(fill) else OUTPUT_FILL, device)
        self.tensor = raw.view(dtype).view(self.shape)
        if not np.isscalar(fill):
            self.tensor.copy_(torch.from_numpy(np.ascontiguousarray(fill)).view(self.shape))

    @property
    def ptr(self):
        return self.tensor.data_ptr()

    def host(self):
        return self.tensor.cpu().numpy()

    def damaged(self):
        return guards_intact(self.whole, self.nbytes)


def only_0_and_1(flags):
    """Whether a host array of flag bytes holds nothing but 0 and 1."""
    return bool((np.asarray(flags).view(np.uint8) <= 1).all())


def first_difference(run, differs, patterns=PATTERNS):
    """Runs ``run(pattern)`` for the patterns in order and stops at the first whose result ``differs(pattern, result)``
    objects to (a message; None or "" when the result is right).  Returns ``(results, failure)``: the results by pattern
    of what was run, and None or ``(pattern, message)`` of the one that stopped it."""
    results = {}
    for pattern in patterns:
        results[pattern] = run(pattern)
        message = differs(pattern, results[pattern])
        if message:
            return results, (pattern, message)
    return results, None
