"""The row-copy kernels of csrc/stream.hip -- k_rows_compact, k_rows_multi, k_rows_packed, k_rows_gather / _scatter --
through their Python entry points, bit for bit against torch indexing on CPU copies: every row width class, sizes on
both sides of every tile, slot, block and grid-cap boundary, aligned and 4-byte-aligned bases, device and pinned
storage, and row lists in any order (tests/row_cases.py).  Sources hold random 32-bit patterns (NaN payloads
included, hence the int32 views); destinations are pre-filled with a sentinel and carry eight guard rows, and the
comparison is of the whole destination, so a word written where none should be fails as a wrong word does."""
import numpy as np
import pytest
import torch

import row_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "f_dc", "opacity", "scaling", "rotation", "f_rest")
WORDS = {"xyz": 3, "f_dc": 3, "opacity": 1, "scaling": 3, "rotation": 4, "f_rest": 45}
SENTINEL = 0x5EA7BEEF
GUARD = 8


def _bits(rows, words, seed, pinned=False):
    """(rows, words) float32 of random 32-bit patterns, on the CPU."""
    a = np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, (rows, words), dtype=np.int64).astype(np.int32)
    t = torch.from_numpy(a).view(torch.float32)
    return t.pin_memory() if pinned else t


def _sentinel(rows, words, where=DEV):
    t = torch.full((rows, words), SENTINEL, dtype=torch.int32).view(torch.float32)
    return t.pin_memory() if where == "pinned" else t.to(where)


def _place(t, where):
    return t.pin_memory() if where == "pinned" else t.to(where)


def _offset_view(rows, words, off, where=DEV):
    """A contiguous (rows, words) sentinel table whose base lies `off` words into a flat buffer (4-byte aligned
    only when off is not a multiple of four), and the buffer."""
    flat = _sentinel(1, off + rows * words + GUARD, where).reshape(-1)
    return flat[off:off + rows * words].view(rows, words), flat


def _same(got, want, what=""):
    g, w = got.detach().cpu().contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = (g != w).reshape(g.shape[0], -1).any(1).nonzero().flatten()
        raise AssertionError(f"{what}: {bad.numel()} rows differ, first {bad[:8].tolist()}")


def _idx(a):
    return torch.from_numpy(np.asarray(a)).long()


def _dev_rows(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def _expect(src_cpu, dst_before, n, src_rows, dst_rows):
    """dst[dst_rows[i]] = src[src_rows[i]], None lists the identity, on CPU copies."""
    want = dst_before.clone()
    s = _idx(src_rows) if src_rows is not None else torch.arange(n)
    d = _idx(dst_rows) if dst_rows is not None else torch.arange(n)
    want[d] = src_cpu[s]
    return want


_sources = {}


def _source(words, rows, where=DEV):
    """One source table per (width, placement), shared by the tests and never written: (CPU copy, placed copy)."""
    key = (words, where)
    if key not in _sources or _sources[key][0].shape[0] < rows:
        cpu = _bits(rows, words, 1000 + words)
        _sources[key] = (cpu, _place(cpu, where))
    cpu, placed = _sources[key]
    return cpu[:rows], placed[:rows]


# ------------------------------------------------------------------------------------------- k_rows_compact
COMPACT_WORDS = (1, 2, 3, 4, 5, 45, 48)
BLOCK_WORDS = 4096  # kCompactChunks * 4: the words one block copies; a thread's four slots lie 1,024 words apart


def compact_sizes(words):
    """n with n * words on, just below and just above: 4 (the tail chunk), 1024 / 2048 / 3072 (which of a thread's
    slots are inside), 4096 (a second block); several blocks; and n = 1."""
    ns = {1, 3 * BLOCK_WORDS // words + 5}
    for b in (4, 1024, 2048, 3072, BLOCK_WORDS):
        ns.update(b // words + d for d in (-1, 0, 1))
    ns = sorted(n for n in ns if n >= 1)
    totals = [n * words for n in ns]
    for b in (4, 1024, 2048, 3072, BLOCK_WORDS):  # each boundary has a size at or below it (one row may exceed 4
        # words) and one less than two rows above
        assert words > b or any(b - 2 * words < t <= b for t in totals)
        assert any(b < t <= b + 2 * words for t in totals)
    return ns


def _compact(words, gen, n, seed):
    from hlgs_core.spt_cache import copy_rows
    rows = RC.source_rows(n)
    src_cpu, src = _source(words, RC.source_rows(3 * BLOCK_WORDS + 8))
    lst = gen(n, rows, seed)
    dst = _sentinel(n + GUARD, words)
    assert dst.data_ptr() % 16 == 0
    copy_rows([(src, dst)], n, _dev_rows(lst), None)
    _same(dst, _expect(src_cpu, _sentinel(n + GUARD, words, "cpu"), n, lst, None),
          f"{gen.__name__} words {words} n {n}")


@pytest.mark.parametrize("words,gen", [pytest.param(w, g, id=f"w{w}-{g.__name__}") for w in COMPACT_WORDS
                                       for g in RC.GENERATORS + ((RC.LIES[w],) if w in RC.LIES else ())])
def test_compact_every_list_and_size(words, gen):
    """copy_rows, device to device, dst_rows=None, aligned destinations: the compaction kernel.  endpoints_lie(w)
    is a list for w-word rows, w = 1 or 2."""
    for n in compact_sizes(words):
        _compact(words, gen, n, seed=n)


@pytest.mark.parametrize("name,n,seed", RC.ADVERSARIAL)
def test_compact_lists_that_deceive_the_end_rows(name, n, seed):
    """The 1-word lists tests/test_row_cases_cpu.py proves to hold a chunk with consecutive-looking end rows and
    other rows between: before the interior rows were looked up, each of these copied rows s0 .. s0 + 3 there.
    Run once against the kernel with the end-row test alone, all ten failed on an MI355X (wrong values, in bounds),
    as did w1-with_repeats and w1-endpoints_lie1 above and the eighteen-table with_repeats case below, and nothing
    else in this file: 2-word rows cannot be deceived (test_row_cases_cpu.py), so endpoints_lie(2) passed there too."""
    _compact(1, RC.BY_NAME[name], n, seed)


@pytest.mark.parametrize("gen", (RC.increasing_dense, RC.permutation, RC.with_repeats), ids=lambda g: g.__name__)
def test_compact_the_caches_eighteen_tables(gen):
    """One call with the cache's 18 tables: 1 to 17 blocks per table, mapped through bstart."""
    from hlgs_core.spt_cache import copy_rows
    n = 1500
    lst = gen(n, RC.source_rows(n), 18)
    widths = [WORDS[k] for k in NAMES * 3]
    srcs = [_bits(RC.source_rows(n), w, 50 + t) for t, w in enumerate(widths)]
    dsts = [_sentinel(n + GUARD, w) for w in widths]
    assert all(d.data_ptr() % 16 == 0 for d in dsts)  # else the call leaves the compaction kernel
    copy_rows([(s.to(DEV), d) for s, d in zip(srcs, dsts)], n, _dev_rows(lst), None)
    for t, (s, d, w) in enumerate(zip(srcs, dsts, widths)):
        _same(d, _expect(s, _sentinel(n + GUARD, w, "cpu"), n, lst, None), f"table {t}")


@pytest.mark.parametrize("empty", ("null", "pointers"))
@pytest.mark.parametrize("widths", ([3, 0, 45, 0, 1], [0, 3, 0, 0, 45, 1, 0]), ids=("middle", "ends_and_pairs"))
def test_compact_with_tables_of_zero_byte_rows(widths, empty):
    """Tables of 0-byte rows have no block (bstart[t] = bstart[t + 1]); the other tables' blocks still find their
    tables, whether an empty table comes first, last, between two others or twice in a row.  "null": through
    copy_rows, which passes NULL for a tensor without elements (torch's data_ptr() of any such tensor, views
    included, is 0); such a table is neither device memory nor anything else, and the dispatcher keeps the call on the
    compaction kernel because the table has no bytes.  "pointers": hlgs_copy_rows called directly, the empty tables
    carrying the device pointers of a real table with row_bytes = 0."""
    from hlgs_core import _lib as L
    from hlgs_core.spt_cache import copy_rows
    n = 2100
    lst = RC.permutation(n, RC.source_rows(n), 2)
    srcs = [_bits(RC.source_rows(n), w, 70 + t) for t, w in enumerate(widths)]
    dsts = [_sentinel(n + GUARD, w) for w in widths]
    pairs = [(s.to(DEV), d) for s, d in zip(srcs, dsts)]
    assert all(d.data_ptr() % 16 == 0 for d in dsts)  # else the call leaves the compaction kernel
    rows = _dev_rows(lst)
    if empty == "null":
        assert all(t.data_ptr() == 0 for (s, d), w in zip(pairs, widths) if not w for t in (s, d))
        copy_rows(pairs, n, rows, None)
    else:
        real = next(p for p, w in zip(pairs, widths) if w)
        tabs = (L.RowCopy * len(pairs))()
        for k, ((s, d), w) in enumerate(zip(pairs, widths)):
            s, d = (s, d) if w else real
            tabs[k] = L.RowCopy(s.data_ptr(), d.data_ptr(), 4 * w)
        L.check(L.load().hlgs_copy_rows(len(pairs), tabs, n, rows.data_ptr(), None, L.stream()))
    for t, (s, d, w) in enumerate(zip(srcs, dsts, widths)):
        _same(d, _expect(s, _sentinel(n + GUARD, w, "cpu"), n, lst, None), f"table {t}")


# ------------------------------------------------------------------------------------------- k_rows_multi, device
MULTI_WORDS = (1, 3, 4, 6, 45)  # with four words per lane, lanes cross row ends at every phase


@pytest.mark.parametrize("n", (1, 5, 257, 1500))
@pytest.mark.parametrize("words", MULTI_WORDS)
def test_multi_both_lists(words, n):
    from hlgs_core.spt_cache import copy_rows
    rows = RC.source_rows(n)
    src_cpu, src = _source(words, rows)
    sl, dl = RC.permutation(n, rows, n), RC.permutation(n, rows, n + 1)
    dst = _sentinel(rows + GUARD, words)
    copy_rows([(src, dst)], n, _dev_rows(sl), _dev_rows(dl))
    _same(dst, _expect(src_cpu, _sentinel(rows + GUARD, words, "cpu"), n, sl, dl))


@pytest.mark.parametrize("gen", (RC.increasing_dense, RC.permutation, RC.with_repeats), ids=lambda g: g.__name__)
@pytest.mark.parametrize("words", MULTI_WORDS)
def test_multi_destination_base_not_16_byte_aligned(words, gen):
    """dst_rows=None, but the destination starts 12 bytes into its buffer (for 3-word rows: the [1:] slice of a
    table), so the compaction kernel's aligned 16-byte stores are not available."""
    from hlgs_core.spt_cache import copy_rows
    for n in (1, 7, 1027):
        src_cpu, src = _source(words, RC.source_rows(n))
        lst = gen(n, RC.source_rows(n), n)
        dst, flat = _offset_view(n + GUARD, words, 3)
        assert dst.data_ptr() % 16 == 12 and dst.is_contiguous()
        copy_rows([(src, dst)], n, _dev_rows(lst), None)
        want, want_flat = _offset_view(n + GUARD, words, 3, "cpu")
        want[:n] = src_cpu[_idx(lst)]
        _same(flat[None], want_flat[None], f"words {words} n {n}")  # the buffer's words around the table too


@pytest.mark.parametrize("T", (21, 32))
def test_multi_more_tables_than_the_compaction_takes(T):
    from hlgs_core.spt_cache import copy_rows
    n = 700
    lst = RC.with_repeats(n, RC.source_rows(n), T)
    widths = [MULTI_WORDS[t % len(MULTI_WORDS)] for t in range(T)]
    srcs = [_bits(RC.source_rows(n), w, 90 + t) for t, w in enumerate(widths)]
    dsts = [_sentinel(n + GUARD, w) for w in widths]
    copy_rows([(s.to(DEV), d) for s, d in zip(srcs, dsts)], n, _dev_rows(lst), None)
    for t, (s, d, w) in enumerate(zip(srcs, dsts, widths)):
        _same(d, _expect(s, _sentinel(n + GUARD, w, "cpu"), n, lst, None), f"table {t}")


def test_multi_grid_stride_second_pass():
    """100,000 rows of 45 words: more than the 4096 x 256 x 4 words one pass of the capped grid covers."""
    from hlgs_core.spt_cache import copy_rows
    n, words = 100_000, 45
    assert n * words > 4096 * 256 * 4
    src_cpu = _bits(n, words, 5)
    sl, dl = RC.permutation(n, n, 1), RC.permutation(n, n, 2)
    dst = _sentinel(n + GUARD, words)
    copy_rows([(src_cpu.to(DEV), dst)], n, _dev_rows(sl), _dev_rows(dl))
    _same(dst, _expect(src_cpu, _sentinel(n + GUARD, words, "cpu"), n, sl, dl))


# ------------------------------------------------------------------------------------------- k_rows_multi, host link
@pytest.mark.parametrize("lists", ("both", "src", "dst", "none"))
@pytest.mark.parametrize("to_host", (False, True), ids=("to_device", "to_host"))
@pytest.mark.parametrize("words", (1, 3, 45))
def test_multi_across_the_host_link(words, to_host, lists):
    """Pinned host memory on one side: one word per lane."""
    from hlgs_core.spt_cache import copy_rows
    for n in (1, 257, 5000):
        rows = RC.source_rows(n)
        src_cpu, src = _source(words, rows, DEV if to_host else "pinned")
        sl = RC.permutation(n, rows, n) if lists in ("both", "src") else None
        dl = RC.permutation(n, rows, n + 1) if lists in ("both", "dst") else None
        dst = _sentinel(rows + GUARD, words, "pinned" if to_host else DEV)
        copy_rows([(src, dst)], n, _dev_rows(sl), _dev_rows(dl))
        torch.cuda.synchronize()
        _same(dst, _expect(src_cpu, _sentinel(rows + GUARD, words, "cpu"), n, sl, dl), f"n {n}")


# ------------------------------------------------------------------------------------------- k_rows_packed
LAYOUTS = {
    "cache18": [WORDS[k] for k in NAMES * 3],              # 177 words in a 768-byte row
    "cache6": [WORDS[k] for k in NAMES],                   # 59 words in 256 bytes
    "prefix3": [1, 3, 3],                                  # 7 words in 64 bytes
    "full256": [45, 45, 45, 45, 48, 16, 4, 4, 3, 1],       # exactly 256 words: a 1,024-byte row without padding
    "ones32": [1] * 32,                                    # every table one word: the smallest row that holds 32
    "ones16": [1] * 16,                                    # a 64-byte row without padding
}
assert sum(LAYOUTS["full256"]) == 256


def _hw(widths):
    return -(-sum(widths) // 16) * 16


def _pack(tables):
    return torch.cat([t.reshape(t.shape[0], -1) for t in tables], 1)


@pytest.mark.parametrize("n", (1, 96, 97, 1000))  # 24 workgroups = 96 waves: at 97 rows a wave takes a second row
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_packed_write_back(layout, n):
    """copy_rows_packed(to_host=True): whole host rows, padding zeroed, other host rows untouched."""
    from hlgs_core.spt_cache import copy_rows_packed
    widths = LAYOUTS[layout]
    hw, H = _hw(widths), RC.source_rows(n)
    dev_cpu = [_bits(H, w, 30 + t) for t, w in enumerate(widths)]
    dev = [t.to(DEV) for t in dev_cpu]
    for dl in (RC.with_repeats(n, H, n), None):
        hl = RC.permutation(n, H, n + 1)
        host = _sentinel(H + GUARD, hw, "pinned")
        copy_rows_packed(dev, n, _dev_rows(dl), _dev_rows(hl), host, to_host=True)
        torch.cuda.synchronize()
        rows = torch.nn.functional.pad(_pack(dev_cpu).view(torch.int32), (0, hw - sum(widths))).view(torch.float32)
        _same(host, _expect(rows, _sentinel(H + GUARD, hw, "cpu"), n, dl, hl), f"dev_rows {dl is not None}")


@pytest.mark.parametrize("n", (8192, 8193))  # 2,048 workgroups = 8,192 waves
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_packed_load(layout, n):
    """copy_rows_packed(to_host=False) and load_rows_packed without resident rows: the tables' parts of the host
    rows, nothing of the padding, and no row past n."""
    from hlgs_core.spt_cache import copy_rows_packed, load_rows_packed
    widths = LAYOUTS[layout]
    hw, H = _hw(widths), n + 100
    host = _bits(H, hw, 40, pinned=True)
    hl = RC.permutation(n, H, n)
    want_rows = host[_idx(hl)][:, :sum(widths)]
    for dl in (None, RC.permutation(n, n, 3)):
        out = [_sentinel(n + GUARD, w) for w in widths]
        copy_rows_packed(out, n, _dev_rows(dl), _dev_rows(hl), host, to_host=False)
        _same(_pack(out), _expect(want_rows, _sentinel(n + GUARD, sum(widths), "cpu"), n, None, dl))
    out = [_sentinel(n + GUARD, w) for w in widths]
    load_rows_packed(out, n, _dev_rows(hl), host)
    _same(_pack(out), _expect(want_rows, _sentinel(n + GUARD, sum(widths), "cpu"), n, None, None))


@pytest.mark.parametrize("resident", ("all", "none", "alternating"))
@pytest.mark.parametrize("layout", ("cache18", "full256", "ones32"))
def test_packed_load_resident_rows(layout, resident):
    """load_rows_packed with resident_of: marked host rows come from the resident tables (whose bits differ from
    the host copy, which proves the source), the others over the host link."""
    from hlgs_core.spt_cache import load_rows_packed
    widths = LAYOUTS[layout]
    n, R = 1000, 600
    hw, H = _hw(widths), RC.source_rows(n)
    host = _bits(H, hw, 41, pinned=True)
    res_cpu = [_bits(R, w, 60 + t) for t, w in enumerate(widths)]
    hl = RC.with_repeats(n, H, 4) if resident == "none" else RC.permutation(n, H, 4)
    of = np.full(H, -1, np.int32)
    if resident != "none":
        marked = np.unique(hl)[::(1 if resident == "all" else 2)]
        of[marked] = np.random.default_rng(6).integers(0, R, marked.size)
    out = [_sentinel(n + GUARD, w) for w in widths]
    load_rows_packed(out, n, _dev_rows(hl), host, [t.to(DEV) for t in res_cpu], _dev_rows(of))
    ro = _idx(of)[_idx(hl)]
    assert {"all": (ro >= 0).all(), "none": (ro < 0).all(), "alternating": 0 < (ro >= 0).sum() < n}[resident]
    rows = torch.where((ro >= 0)[:, None], _pack(res_cpu).view(torch.int32)[ro.clamp(min=0)],
                       host[_idx(hl)][:, :sum(widths)].view(torch.int32)).view(torch.float32)
    _same(_pack(out), _expect(rows, _sentinel(n + GUARD, sum(widths), "cpu"), n, None, None))


# ------------------------------------------------------------------------------------------- k_rows_gather / _scatter
GATHER_N = (1, 15, 16, 17, 5000)  # 16 rows per block


def _gather_cases():
    for where in (DEV, "pinned"):
        for words in (1, 3, 4, 8, 45):
            yield pytest.param(words, where, 0, 0, id=f"w{words}-{where}")
            if words in (4, 8):  # rows of whole 16 bytes: the float4 kernel above, the uint32_t kernel below
                yield pytest.param(words, where, 1, 0, id=f"w{words}-{where}-storage+4")
                yield pytest.param(words, where, 0, 1, id=f"w{words}-{where}-rows+4")


@pytest.mark.parametrize("words,where,storage_off,rows_off", list(_gather_cases()))
def test_gather_rows(words, where, storage_off, rows_off):
    from hlgs_core import spt
    for n in GATHER_N:
        P = RC.source_rows(n)
        flat_cpu = _bits(1, storage_off + P * words, 80 + words).reshape(-1)
        flat = _place(flat_cpu, where)
        storage = flat[storage_off:].view(P, words)
        assert storage.data_ptr() % 16 == 4 * storage_off
        idx = torch.from_numpy(RC.with_repeats(n, P, n) if n > 1 else RC.permutation(n, P, n)).long()
        out, out_flat = _offset_view(n + GUARD, words, rows_off)
        got = spt.gather_rows(storage, idx.to(DEV), out=out[:n])
        assert got.data_ptr() == out.data_ptr()
        want, want_flat = _offset_view(n + GUARD, words, rows_off, "cpu")
        want[:n] = flat_cpu[storage_off:].view(P, words)[idx]
        _same(out_flat[None], want_flat[None], f"n {n}")
    got = spt.gather_rows(storage, idx.to(DEV))  # the allocating form
    _same(got, flat_cpu[storage_off:].view(P, words)[idx])


@pytest.mark.parametrize("words,where,storage_off,rows_off", list(_gather_cases()))
def test_scatter_rows(words, where, storage_off, rows_off):
    from hlgs_core import spt
    for n in GATHER_N:
        P = RC.source_rows(n)
        storage, flat = _offset_view(P + GUARD, words, storage_off, where)
        vals_cpu = _bits(1, rows_off + n * words, 85 + words).reshape(-1)
        vals = vals_cpu.to(DEV)[rows_off:].view(n, words)
        assert vals.data_ptr() % 16 == 4 * rows_off and vals.is_contiguous()
        idx = torch.from_numpy(RC.permutation(n, P, n)).long()
        spt.scatter_rows(storage, idx.to(DEV), vals)
        torch.cuda.synchronize()
        want, want_flat = _offset_view(P + GUARD, words, storage_off, "cpu")
        want[idx] = vals_cpu[rows_off:].view(n, words)
        _same(flat[None], want_flat[None], f"n {n}")
