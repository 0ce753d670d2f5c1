"""Guard frames around kernel outputs: a window of a larger, pattern-filled buffer, and the check that nothing outside the window changed.

A write one chunk past column N of row m of an exact-fit [M, N] tensor lands in row m + 1 of the same tensor, where it is overwritten by
(or races with) the right value: no comparison of y with a reference can see it.  A Frame puts y anywhere a caller may put it - a row
stride above N, a column slice of a wider buffer, a base that is 8- but not 16-byte aligned - inside one flat allocation whose every byte
outside the window is known, so a stray write has an observer.

    f = Frame(rows, cols, ld, col_off, elem_off, dtype, device, guard_rows)
    kernel(..., f.view.data_ptr(), f.view.stride(0), ...)
    f.assert_untouched("what ran")

The GEMMs choose their store path from three properties of y (gemm_wreg.hip, and its copies in gemm.hip, gemm_sk.hip, gemm_w8a16.hip):
    staged = (N % 8 == 0) && (ldy % 8 == 0) && (y % 16 == 0)
store_class() restates that selector and LAYOUTS(N) is the fixed list of output layouts every GEMM test runs;
tests/test_frames_host.py shows that the list reaches every class for each N the GPU tests use, and that the frame check has teeth."""
import torch

GUARD_ROWS = 256                 # the tallest tile of _capi.gemm_config_names() (test_frames_host.py reads the table)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


_patterns = {}                   # device -> the longest pattern made so far (a prefix serves every shorter buffer)


def _pattern(n16, device="cpu"):
    """Position-dependent 16-bit values (an odd multiplier: 65536 consecutive positions all differ), so a stray write of ANY constant,
    zero included, changes something."""
    key = str(device)
    have = _patterns.get(key)
    if have is None or have.numel() < n16:
        i = torch.arange(max(n16, 1 << 20), dtype=torch.int64, device=device)
        v = (i * 40503 + 0x5A17) & 0xFFFF
        have = _patterns[key] = torch.where(v >= 0x8000, v - 0x10000, v).to(torch.int16)
    return have[:n16]


class Frame:
    """One flat buffer filled with the pattern; `.view` is the [rows, cols] window with row stride `ld` (elements of `dtype`) that starts at
    column `col_off` of a row grid whose origin lies `elem_off` elements behind a 256-byte boundary.  At least `guard_rows` full rows
    of guard lie in front of the window and behind it; the columns [cols, ld) of every row are guard too."""

    def __init__(self, rows, cols, ld, col_off=0, elem_off=0, dtype=torch.float16, device="cpu", guard_rows=GUARD_ROWS):
        assert rows >= 0 and cols >= 0 and col_off >= 0 and elem_off >= 0 and guard_rows >= 1
        assert col_off + cols <= ld, "the window does not fit its row"
        self.rows, self.cols, self.ld, self.col_off, self.elem_off, self.dtype = rows, cols, ld, col_off, elem_off, dtype
        es = torch.empty(0, dtype=dtype).element_size()
        self.itype = _INT[es]
        per256 = 256 // es
        pre = -(-guard_rows * ld // per256) * per256                      # whole 256-byte units: the row grid's origin keeps the boundary
        total = (per256 + pre + elem_off + (rows + guard_rows) * ld + per256 + 1) & ~1
        raw = torch.empty(total * es // 2 + 1, dtype=torch.int16, device=device)
        raw.copy_(_pattern(raw.numel(), device))
        self.raw = raw
        flat = raw[: total * es // 2].view(dtype)
        skew = (-flat.data_ptr() % 256) // es                               # (allocators align to 256 bytes and more; not relied on)
        self.flat = flat
        self.start = skew + pre + elem_off + col_off                      # flat index of window element (0, 0)
        assert (flat.data_ptr() + (self.start - col_off - elem_off) * es) % 256 == 0
        self.view = flat.as_strided((rows, cols), (ld, 1), self.start)
        self.saved = raw.clone()
        self._outside = torch.ones(flat.numel(), dtype=torch.bool, device=device)
        self._outside.as_strided((rows, cols), (ld, 1), self.start).fill_(False)

    def reset(self):
        """Back to the saved bytes (the pattern, or what freeze() kept): the same frame serves the next launch."""
        self.raw.copy_(self.saved)

    def freeze(self):
        """Keep the buffer as it is now - the window filled by the caller - as the saved image: for an INPUT operand, whose window must not
        change either (assert_unchanged)."""
        self.saved = self.raw.clone()
        return self

    def assert_unchanged(self, what):
        """Window and guard alike equal the saved image."""
        self.assert_untouched(what)
        if not torch.equal(self.raw, self.saved):
            raise AssertionError(f"{what}: the [{self.rows}, {self.cols}] window itself changed (an input operand)")

    def saved_view(self):
        """The window as it was filled (the pattern), for callers that check parts of the window itself."""
        return self.saved[: self.flat.numel() * self.flat.element_size() // 2].view(self.dtype).as_strided((self.rows, self.cols), (self.ld, 1), self.start)

    def assert_untouched(self, what):
        """Every byte outside the window equals the saved pattern; else name the first offending (row, column) relative to the window
        (column in [0, ld): columns >= cols are the row's pad, negative rows lie in front of the window) and the number of changed elements."""
        n = self.flat.numel()
        now = self.flat.view(self.itype)
        was = self.saved[: n * self.flat.element_size() // 2].view(self.itype)
        tail_ok = bool(torch.equal(self.raw[-1:], self.saved[-1:]))
        bad = (now != was) & self._outside
        count = int(bad.sum())
        if count or not tail_ok:
            i = int(torch.nonzero(bad.reshape(-1))[0]) if count else n
            rel = i - self.start
            row, col = rel // self.ld, rel % self.ld
            raise AssertionError(f"{what}: {count} element(s) outside the [{self.rows}, {self.cols}] window (ld {self.ld}, column offset {self.col_off}, "
                                 f"element offset {self.elem_off}) changed; first at (row {row}, column {col}) relative to the window")


def store_class(N, ld, ptr):
    """The GEMMs' store-path selector restated (N: the output's column count - N / 2 for MIXQ_ACT_SILU_PAIR; ld in elements; ptr: the byte
    address of y[0, 0]): 'staged', or the first reason the direct 8-byte stores are taken."""
    if N % 8:
        return "unstaged_by_N"
    if ld % 8:
        return "unstaged_by_ld"
    if ptr % 16:
        return "unstaged_by_ptr"
    return "staged"


def LAYOUTS(N):
    """(ld, col_off, elem_off) of every output layout a GEMM test runs, in elements."""
    return [(N, 0, 0),                    # exact fit
            (N + 8, 0, 0),                # a pad, still staged
            (2 * N + 64, N + 8, 0),       # a column slice of a wide buffer (q/k/v, gate/up written into one tensor)
            (N + 4, 0, 0),                # ld % 8 == 4
            (N + 8, 0, 4),                # a base that is 8-byte but not 16-byte aligned
            (N + 4, 4, 0)]                # both


def layout_ptr(layout):
    """Byte address of y[0, 0] modulo 256 for a 16-bit Frame in `layout` (what store_class needs without allocating)."""
    _, col_off, elem_off = layout
    return (2 * (col_off + elem_off)) % 256


def classes_possible(N):
    """The classes store_class can return for this N."""
    return {"unstaged_by_N"} if N % 8 else {"staged", "unstaged_by_ld", "unstaged_by_ptr"}
