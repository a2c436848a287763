"""A controlled `regtr_amd.ops._ws`: every workspace a launcher is handed is the middle of a larger buffer, pre-filled with a chosen
byte pattern and fenced by sentinel guard bands (tests/test_gpu_workspace_leftovers.py).  Importing this needs no GPU.

    with PoisonedWorkspaces('ones') as hook:
        out = ops.instnorm_stats(...)
    hook.check()                      # every guard band still holds the sentinel
    assert hook.served(nbytes)        # a request of exactly that size was made

The fills: 'zeros' 0x00; 'ones' 0xFF (NaN as float32 / float64, -1 as an integer); 'x7f' 0x7F (a large finite float, a large positive
integer); 'random' seeded random bytes drawn on the device (another kernel's leftovers).  The sentinel byte differs from all three
constant fills.  Every request gets a buffer of its own, kept by the hook until it is dropped, so no two live requests share memory."""
import torch

FILLS = ('zeros', 'ones', 'x7f', 'random')
FILL_BYTE = {'zeros': 0x00, 'ones': 0xFF, 'x7f': 0x7F}
SENTINEL = 0xA5
GUARD_BYTES = 4096
ALIGN = 256            # what torch.empty gives a fresh allocation; the launchers carve 256-byte aligned sub-buffers from it

assert SENTINEL not in FILL_BYTE.values() and GUARD_BYTES >= 4096 and GUARD_BYTES % ALIGN == 0


class PoisonedWorkspaces:
    """Context manager: replaces ops._ws for its duration.  `requests` is the list of (nbytes, served view) in call order."""

    def __init__(self, fill, seed=0, guard=GUARD_BYTES):
        if fill not in FILLS:
            raise ValueError(f'fill must be one of {FILLS}, got {fill!r}')
        if guard < GUARD_BYTES:
            raise ValueError(f'the guard bands are at least {GUARD_BYTES} bytes')
        self.fill, self.seed, self.guard = fill, int(seed), int(guard)
        self.requests = []
        self._records = []             # (whole buffer, offset of the served bytes, nbytes)
        self._orig = None

    # -------------------------------------------------------------------------------------------- the allocator
    def _alloc(self, nbytes, device):
        n = int(nbytes)
        if n < 0:
            raise ValueError(f'a workspace of {n} bytes was asked for')
        whole = torch.full((n + 2 * self.guard + ALIGN,), SENTINEL, dtype=torch.uint8, device=device)
        off = self.guard + (-(whole.data_ptr() + self.guard)) % ALIGN
        view = whole[off:off + n]
        assert view.data_ptr() % ALIGN == 0 and off >= self.guard and whole.numel() - (off + n) >= self.guard
        if self.fill == 'random':
            gen = torch.Generator(device=whole.device)
            gen.manual_seed(self.seed + len(self._records))
            view.copy_(torch.randint(0, 256, (n,), dtype=torch.uint8, device=whole.device, generator=gen))
        else:
            view.fill_(FILL_BYTE[self.fill])
        self._records.append((whole, off, n))
        self.requests.append((n, view))
        return view

    def __enter__(self):
        from regtr_amd import ops
        if self._orig is not None:
            raise RuntimeError('PoisonedWorkspaces is not re-entrant')
        self._orig, ops._ws = ops._ws, self._alloc
        return self

    def __exit__(self, *exc):
        from regtr_amd import ops
        ops._ws, self._orig = self._orig, None
        return False

    # -------------------------------------------------------------------------------------------- what the tests ask
    def sizes(self):
        return [n for n, _ in self.requests]

    def served(self, nbytes):
        """How many requests asked for exactly `nbytes` bytes."""
        return self.sizes().count(int(nbytes))

    def check(self):
        """Every guard band of every request still holds the sentinel (synchronises)."""
        for k, (whole, off, n) in enumerate(self._records):
            lead, trail = whole[:off], whole[off + n:]
            bad_lead, bad_trail = int((lead != SENTINEL).sum()), int((trail != SENTINEL).sum())
            assert bad_lead == 0 and bad_trail == 0, (f'request {k} ({n} bytes, fill {self.fill}): {bad_lead} bytes written before the workspace, '
                                                      f'{bad_trail} past its end')
        return len(self._records)
