"""Shared cases of the operators that touch a relation before the engine does (include/skfusion_hip.h: skf_fill_unknown,
skf_cast, skf_to_bf16, skf_fill_uniform), called through the C ABI on whichever runtime is installed:
tests/test_preprocess_emul.py runs them on the host emulator, tests/test_gpu_preprocess.py on the MI355X.

Every case runs between guard bands (tests/guarded.py) and every device matrix is a `Held`: its rows lie `ld` elements apart,
the elements beyond the width hold POISON bytes before the call and must hold them after it.

SEAMS are the smallest shapes at which each loop of these kernels turns over: (1, 1); (5, 64), (5, 65), (3, 131) the 64-lane
column loop of a row and its tail; (257, 3) the second trip of fill_total_kernel's 256 threads; (33, 31), (32, 32), (65, 97)
the 32 x 32 tile seams of the transposed conversion; (8209, 67) more rows than a wave_grid launch holds (8192) and more
elements than an elem_grid launch holds (524 288); (2, 524 301) more columns than an elem_grid launch of
fill_col_stats_kernel holds.

References, none of them the code under test:
  fill_model   a NumPy statement of the header's rules in f64 (sums in np.longdouble where the data is not exact), itself held
               to the reference's recorded outputs in tests/golden/fill_strategies.npz;
  bf16_rne     round-to-nearest-even on the bit pattern, compare-based integer arithmetic on uint64, NaN stated apart;
  ndarray.astype of NumPy for the casts; oracle.hash_uniform_matrix for the generator."""
import ctypes as C

import numpy as np

import skfusion_amd._native as nat
from guarded import guarded
from helpers import golden, within

F64, F32, BF16 = nat.SKF_F64, nat.SKF_F32, nat.SKF_BF16
NPD = {F64: np.float64, F32: np.float32, BF16: np.uint16}
POISON = 0xA5
SEAMS = [(1, 1), (5, 64), (5, 65), (3, 131), (257, 3), (33, 31), (32, 32), (65, 97), (8209, 67), (2, 524301)]
LARGE = [(8209, 67), (2, 524301)]           # the emulator runs these too: every case under ten seconds there
STRUCTURE_SHAPES = [(8209, 67), (131, 257)]
REAL_SHAPES = [(8209, 67), (2, 524301)]
MEAN, ROW_MEAN, COL_MEAN, CONST = 0, 1, 2, 3
STRATEGIES = (MEAN, ROW_MEAN, COL_MEAN, CONST)
CONST_VALUE = -2.625
Y_EXTENT = (2097185, 3)                      # 65 537 tiles of 32 rows: past 65 535 and past 65 536
REPORT = []                                  # lines for profiles/preprocess_ops.txt (printed by the modules' last test)


def pad64(n):
    return (n + 63) // 64 * 64


def shape_id(shape):
    return '%dx%d' % shape


def seed_of(rows, cols, k):
    return (rows * 1000003 + cols * 101 + k) % (2 ** 31)


class Held(object):
    """A rows x cols matrix on the device, rows `ld` elements apart, inside an upload of exactly rows * ld elements whose
    other bytes are `fill` (POISON; 0 where the caller's promise is 'zeroed padding stays zero').  X=None: the matrix itself
    holds `fill` too (an output: an element the operator does not write keeps it and fails the comparison)."""

    def __init__(self, mem, X, ld, dtype=None, shape=None, fill=POISON):
        if X is not None:
            X = np.ascontiguousarray(X)
            dtype, shape = X.dtype, X.shape
        self.mem, self.shape, self.ld, self.dtype = mem, shape, int(ld), np.dtype(dtype)
        rows, cols = shape
        assert ld >= cols
        self.host = np.full(max(rows * self.ld, 1) * self.dtype.itemsize, fill, np.uint8)
        if X is not None and X.size:
            self._matrix(self.host)[:, :cols] = X
        self.buf = mem.from_host(self.host)
        self.ptr = self.buf.ptr

    def _matrix(self, raw):
        return raw[:self.shape[0] * self.ld * self.dtype.itemsize].view(self.dtype).reshape(self.shape[0], self.ld)

    def raw(self):
        self.mem.synchronize()
        return self.mem.to_host(self.buf, self.host.shape, np.uint8)

    def download(self):
        """The matrix after the call; asserts that every byte beyond the width still holds what it held."""
        got, cols = self.raw(), self.shape[1]
        np.testing.assert_array_equal(self._matrix(got)[:, cols:], self._matrix(self.host)[:, cols:],
                                      err_msg='padding columns changed')
        return self._matrix(got)[:, :cols].copy()

    def unchanged(self, what=''):
        np.testing.assert_array_equal(self.raw(), self.host, err_msg='%s: buffer changed' % what)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view('u%d' % a.dtype.itemsize)


def same_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def same_values(got, want, what, nan_sign=True):
    """Bit for bit where `want` is not NaN; where it is: NaN, of the same sign where the sign is an input's (`nan_sign`; the
    sign of a NaN that arithmetic makes, inf - inf or 0 / 0, is the processor's choice)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg='%s: NaN positions' % what)
    if nan_sign:
        np.testing.assert_array_equal(np.signbit(got[nan]), np.signbit(want[nan]), err_msg='%s: NaN signs' % what)
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan], err_msg='%s: values' % what)


# ---------------------------------------------------------------------------------------------------------------------------
# skf_fill_unknown
# ---------------------------------------------------------------------------------------------------------------------------
class Filled(object):
    """What fill_model returns: .out the filled matrix (f64), .unknown the entries replaced, the statistics of the workspace
    layout (.row_sum, .row_cnt, .col_sum, .col_cnt, .tot_sum, .tot_cnt), the sums of |x| beside them (.row_abs, .col_abs,
    .tot_abs) and .bound, per entry the first-order bound of a mean of n terms summed in any order and divided once:
    (n + 2) 2^-53 sum|x| / count."""


def fill_model(X, mask, strategy, value=0.0, acc=np.float64):
    """include/skfusion_hip.h, skf_fill_unknown: an entry is KNOWN when it is neither masked nor NaN -- +-inf are known to
    the means --; every entry that is masked or not finite is replaced: by the mean of all known entries (0), of its row (1),
    of its column (2) -- a line without a usable mean takes the overall one; usable = finite when a mask is given, not NaN
    when none is --, or by `value` (3).  Nothing known: 0 / 0 = NaN.  `mask` None is 'no mask given', an array of zeros is a
    mask.  Sums in `acc`, one division, rounded to f64."""
    X = np.asarray(X, dtype=np.float64)
    hidden = np.zeros(X.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    known = ~hidden & ~np.isnan(X)
    m = Filled()
    m.unknown = hidden | ~np.isfinite(X)
    Z = np.where(known, X, 0.0).astype(acc)
    A = np.where(known & np.isfinite(X), np.abs(X), 0.0).astype(acc)
    u = 2.0 ** -53
    with np.errstate(all='ignore'):
        m.row_sum, m.row_cnt = Z.sum(axis=1), known.sum(axis=1)
        m.col_sum, m.col_cnt = Z.sum(axis=0), known.sum(axis=0)
        m.tot_sum, m.tot_cnt = Z.sum(), int(known.sum())
        m.row_abs, m.col_abs, m.tot_abs = A.sum(axis=1), A.sum(axis=0), A.sum()
        overall = np.float64(m.tot_sum / acc(m.tot_cnt)) if m.tot_cnt else np.float64(np.nan)
        overall_bound = (m.tot_cnt + 2) * u * float(m.tot_abs) / max(m.tot_cnt, 1)
        if strategy == MEAN:
            fill, bound = np.full(X.shape, overall), np.full(X.shape, overall_bound)
        elif strategy == CONST:
            fill, bound = np.full(X.shape, np.float64(value)), np.zeros(X.shape)
        else:
            s, n, a = ((m.row_sum, m.row_cnt, m.row_abs) if strategy == ROW_MEAN else (m.col_sum, m.col_cnt, m.col_abs))
            line = (s / np.maximum(n, 1).astype(acc)).astype(np.float64)
            line[n == 0] = np.nan
            usable = np.isfinite(line) if mask is not None else ~np.isnan(line)
            line = np.where(usable, line, overall)
            lb = np.where(usable, (n + 2) * u * a.astype(np.float64) / np.maximum(n, 1), overall_bound)
            along = (lambda v: v[:, None]) if strategy == ROW_MEAN else (lambda v: v[None, :])
            fill, bound = np.broadcast_to(along(line), X.shape), np.broadcast_to(along(lb), X.shape)
    m.out = np.where(m.unknown, fill, X)
    m.bound = np.where(m.unknown, bound, 0.0)
    for name in ('row_sum', 'col_sum', 'tot_sum', 'row_abs', 'col_abs', 'tot_abs'):
        setattr(m, name, np.asarray(getattr(m, name), dtype=np.float64))
    return m


GOLDEN_TAGS = ('masked', 'plain', 'finite', 'corner', 'plaincorner', 'nomask', 'nomaskfinite', 'maskedinf')
GOLDEN_FILLS = (('mean', MEAN), ('row_mean', ROW_MEAN), ('col_mean', COL_MEAN), ('0.5', CONST))


def model_against_golden():
    """fill_model on the eight inputs and four fills of tests/golden/fill_strategies.npz, the reference's recorded outputs:
    every entry bit for bit, a NaN as a NaN.  The mask goes in as the class layer hands it on: only when it masks something.
    One rule of numpy.ma is not the operator's and is left out of the comparison: a MaskedArray that masks nothing hands the
    entries of a line with an INFINITE mean back masked with 1 beneath (tag 'nomask'; the class layer fills that shape on the
    host); those entries are the golden's own output mask.  Returns the number of entries compared."""
    z = golden('fill_strategies.npz')
    n = 0
    for tag in GOLDEN_TAGS:
        if tag.startswith('plain'):
            X, mask = z[tag], None
        else:
            X, mask = z[tag + '_data'], z[tag + '_mask']
            mask = mask if mask.any() else None
        for name, strategy in GOLDEN_FILLS:
            want = z['%s/%s/data' % (tag, name)]
            skip = np.zeros(X.shape, dtype=bool)
            if tag.startswith('nomask') and strategy in (ROW_MEAN, COL_MEAN):
                skip = z['%s/%s/mask' % (tag, name)]
            got = fill_model(X, mask, strategy, 0.5).out
            what = 'model against golden %s/%s' % (tag, name)
            same_values(got[~skip], want[~skip], what, nan_sign=False)
            n += int((~skip).sum())
    return n


def run_fill(rt, dtype, X, mask, strategy, pad, value=CONST_VALUE):
    """skf_fill_unknown on X (f64 values, stored as `dtype`) with ld = cols + pad and mask_ld = cols + pad + 2 when pad > 0.
    Returns (the matrix after the call, the workspace as f64 words, the workspace as uploaded); padding is checked."""
    rows, cols = X.shape
    x = Held(rt.mem, X.astype(NPD[dtype]), cols + pad)
    m = None if mask is None else Held(rt.mem, np.asarray(mask, dtype=np.uint8), cols + (pad + 2 if pad else 0))
    need = C.c_size_t()
    rt.call('skf_fill_unknown_workspace_bytes', rows, cols, C.byref(need))
    assert need.value == (2 * rows + 2 * cols + 2) * 8
    ws = Held(rt.mem, None, need.value, np.uint8, (1, need.value))
    rt.call('skf_fill_unknown', dtype, x.ptr, x.ld, rows, cols, m.ptr if m else None, m.ld if m else 0, strategy, float(value),
            ws.ptr, need.value, None)
    got = x.download()
    if m is not None:
        m.unchanged('mask')
    return got, ws.raw().view(np.float64), ws.host.view(np.float64)


def check_stats(stats, blank, model, strategy, rows, cols, exact, what):
    """The statistics layout of the workspace: row sums, row counts, column sums, column counts (written for col_mean only),
    total sum, total count; the words a strategy does not write keep their bytes.  Counts are exact integers; sums exact
    when the data is (`exact`), else within the bound of a sum of n terms in any order."""
    if strategy == CONST:
        same_bits(stats, blank, what + ': a constant fill writes no statistics')
        return
    pieces = [('row sums', 0, rows, model.row_sum, model.row_cnt, model.row_abs),
              ('total sum', 2 * rows + 2 * cols, 1) + tuple(np.atleast_1d(v) for v in (model.tot_sum, model.tot_cnt, model.tot_abs))]
    if strategy == COL_MEAN:
        pieces.append(('column sums', 2 * rows, cols, model.col_sum, model.col_cnt, model.col_abs))
    else:
        same_bits(stats[2 * rows:2 * rows + 2 * cols], blank[2 * rows:2 * rows + 2 * cols], what + ': column statistics written')
    for name, at, n, sums, counts, abs_sums in pieces:
        got_s, got_n = stats[at:at + n], stats[at + n:at + 2 * n]
        np.testing.assert_array_equal(got_n, np.asarray(counts, dtype=np.float64), err_msg='%s: counts, %s' % (what, name))
        if exact:
            same_values(got_s, sums, '%s: %s' % (what, name), nan_sign=False)
        else:
            ok = np.abs(got_s - sums) <= np.asarray(counts) * 2.0 ** -53 * abs_sums
            assert ok.all(), '%s: %s beyond n 2^-53 sum|x|' % (what, name)


def check_exact_fill(rt, dtype, X, mask, strategy, pad, what):
    """One call on data whose every partial sum is exact in f64: f64 result = the model bit for bit, f32 result = np.float32 of
    the model's f64 fill with the known entries untouched; non-finite expectations as 'same infinity' / 'both NaN'."""
    rows, cols = X.shape
    model = fill_model(X, mask, strategy, CONST_VALUE)
    got, stats, blank = run_fill(rt, dtype, X, mask, strategy, pad)
    npd = NPD[dtype]
    want = np.where(model.unknown, model.out.astype(npd), X.astype(npd))
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what + ': NaN positions')
    same_bits(got[~nan], want[~nan], what)
    check_stats(stats, blank, model, strategy, rows, cols, True, what)
    return model


def exact_data(rs, rows, cols, kind):
    """Entries k / 8, k = 1 .. 64; kind: 'neither', 'nan' (about 10 % NaN), 'mask' (about 10 % masked), 'both'."""
    X = rs.randint(1, 65, size=(rows, cols)) / 8.0
    mask = None
    if kind in ('nan', 'both'):
        X[rs.rand(rows, cols) < 0.1] = np.nan
    if kind in ('mask', 'both'):
        mask = rs.rand(rows, cols) < 0.1
    return X, mask


KINDS = ('neither', 'nan', 'mask', 'both')


def fill_exact_case(shape, dtype, kind, strategies=STRATEGIES):
    rows, cols = shape
    X, mask = exact_data(np.random.RandomState(seed_of(rows, cols, KINDS.index(kind))), rows, cols, kind)
    with guarded() as g:
        for strategy in strategies:
            for pad in (0, 3):
                check_exact_fill(g.rt, dtype, X, mask, strategy, pad,
                                 'fill %s %s strategy %d ld cols + %d' % (shape_id(shape), kind, strategy, pad))


def structure_inputs(shape):
    """name -> (X, mask): the corners of the rules at a shape where the special lines lie past row 8192 (where the shape has
    them) and past column 64; k / 8 data, so every expectation is exact."""
    rows, cols = shape
    rs = np.random.RandomState(seed_of(rows, cols, 77))
    r_none, r_pinf, r_both, r_ninf = rows - 3, rows - 5, rows - 6, rows - 8
    c_none, c_pinf, c_both = cols - 2, cols - 1, cols - 3
    out = {}

    def base(masked):
        X, mask = exact_data(rs, rows, cols, 'both' if masked else 'nan')
        for r in (r_pinf, r_both, r_ninf):                 # the lines under test keep entries to fill
            X[r, 1] = np.nan
        X[1, c_pinf] = X[1, c_both] = np.nan
        if masked:
            mask[r_pinf, 1] = mask[1, c_pinf] = False
        return X, mask
    for masked in (False, True):
        tag = ' under a mask' if masked else ''
        X, mask = base(masked)
        X[r_none, :] = np.nan
        if masked:
            mask[:, c_none] = True                         # (finite data beneath)
        else:
            X[:, c_none] = np.nan
        out['a row and a column without a known entry' + tag] = (X, mask)
        X, mask = base(masked)
        X[r_pinf, 3] = X[4, c_pinf] = np.inf
        if masked:
            mask[r_pinf, 3] = mask[4, c_pinf] = False
        out['a row and a column holding +inf only' + tag] = (X, mask)
        X, mask = base(masked)
        X[r_pinf, 3], X[r_ninf, 5], X[r_both, 2], X[r_both, 7] = np.inf, -np.inf, np.inf, -np.inf
        X[4, c_pinf], X[6, c_both], X[9, c_both] = np.inf, np.inf, -np.inf
        if masked:
            for r, c in ((r_pinf, 3), (r_ninf, 5), (r_both, 2), (r_both, 7), (4, c_pinf), (6, c_both), (9, c_both)):
                mask[r, c] = False
        out['lines holding +inf, -inf and both' + tag] = (X, mask)
    X, _ = exact_data(rs, rows, cols, 'neither')
    out['nothing known: NaN throughout'] = (np.full(shape, np.nan), None)
    out['nothing known: masked throughout'] = (X, np.ones(shape, dtype=bool))
    out['no unknown entry'] = (X, None)
    out['no unknown entry under a mask of zeros'] = (X, np.zeros(shape, dtype=bool))
    return out


def fill_structure_case(shape, dtype):
    with guarded() as g:
        for name, (X, mask) in sorted(structure_inputs(shape).items()):
            for strategy in STRATEGIES:
                for pad in (0, 3):
                    what = 'fill %s, %s, strategy %d, ld cols + %d' % (shape_id(shape), name, strategy, pad)
                    model = check_exact_fill(g.rt, dtype, X, mask, strategy, pad, what)
                    if name.startswith('no unknown'):
                        assert not model.unknown.any()
                    if name.startswith('nothing known') and strategy != CONST:
                        assert np.isnan(model.out).all()
    # the structure inputs do what their names say
    s = structure_inputs(shape)
    X, mask = s['lines holding +inf, -inf and both']
    plain, under = fill_model(X, None, ROW_MEAN), fill_model(*s['lines holding +inf, -inf and both under a mask'], strategy=ROW_MEAN)
    assert np.isnan(plain.tot_sum) and np.isposinf(plain.out[shape[0] - 5, 1]) and np.isneginf(plain.out[shape[0] - 8, 1])
    assert np.isnan(under.out[shape[0] - 5, 1]) and np.isnan(under.out[shape[0] - 8, 1])


def fill_real_case(shape, dtype, label):
    """rand - 0.3 with about 10 % NaN and about 10 % masked: every filled entry within (n + 2) 2^-53 sum|x| / count of the
    model (n the entries summed for that mean; the model sums in np.longdouble, so the bound is the device's alone), f32 plus
    2^-24 |fill| for the rounding of the stored value; known entries bit for bit."""
    rows, cols = shape
    rs = np.random.RandomState(seed_of(rows, cols, 5))
    X = rs.rand(rows, cols) - 0.3
    npd = NPD[dtype]
    X = X.astype(npd).astype(np.float64)                    # the values as stored
    X[rs.rand(rows, cols) < 0.1] = np.nan
    mask = rs.rand(rows, cols) < 0.1
    with guarded() as g:
        for strategy in (MEAN, ROW_MEAN, COL_MEAN):
            for pad in (0, 3):
                model = fill_model(X, mask, strategy, acc=np.longdouble)
                got, stats, blank = run_fill(g.rt, dtype, X, mask, strategy, pad)
                what = '%s fill %s %s strategy %d ld cols + %d' % (label, shape_id(shape), nat_name(dtype), strategy, pad)
                same_bits(got[~model.unknown], X.astype(npd)[~model.unknown], what + ': known entries')
                bound = model.bound + (2.0 ** -24 * np.abs(model.out) if dtype == F32 else 0.0)
                err = np.abs(got.astype(np.longdouble) - model.out)[model.unknown]
                assert np.isfinite(err).all(), what
                ratio = float((err / bound[model.unknown]).max())
                within(ratio, 1.0, what + ', |got - model| / bound')
                REPORT.append('%-70s worst |got - model| / bound %.3e (largest bound %.3e, largest |got - model| %.3e)'
                              % (what, ratio, float(bound[model.unknown].max()), float(err.max())))
                check_stats(stats, blank, model, strategy, rows, cols, False, what)


def nat_name(dtype):
    return {F64: 'f64', F32: 'f32', BF16: 'bf16'}[dtype]


def fill_refusals_case():
    """Every refusal returns its code and leaves data, mask and workspace as they were; rows == 0 or cols == 0 is SKF_OK
    without a launch."""
    from skfusion_amd._engine import launch_count
    rows, cols = 9, 7
    X, mask = exact_data(np.random.RandomState(3), rows, cols, 'both')
    with guarded() as g:
        rt, lib = g.rt, g.rt.lib
        x, m = Held(rt.mem, X, cols + 3), Held(rt.mem, mask.astype(np.uint8), cols + 5)
        need = (2 * rows + 2 * cols + 2) * 8
        ws = Held(rt.mem, None, need, np.uint8, (1, need))
        E, W = nat.SKF_E_INVALID, nat.SKF_E_WORKSPACE

        def call(dtype=F64, data=x.ptr, ld=x.ld, r=rows, c=cols, msk=m.ptr, mld=m.ld, strategy=ROW_MEAN, wsp=ws.ptr, wsb=need):
            before = launch_count(rt)
            rc = lib.skf_fill_unknown(dtype, data, ld, r, c, msk, mld, strategy, 0.0, wsp, wsb, None)
            assert launch_count(rt) == before, 'a refused or empty call launched a kernel'
            x.unchanged('data'), m.unchanged('mask'), ws.unchanged('workspace')
            return rc
        assert call(ld=cols - 1) == E
        assert call(mld=cols - 1) == E
        assert call(strategy=-1) == E and call(strategy=4) == E
        assert call(dtype=BF16) == E and call(dtype=7) == E
        assert call(r=-1) == E and call(c=-1) == E
        assert call(wsb=need - 1) == W
        assert call(wsp=None) == W
        assert call(data=None) == E
        assert call(msk=None, mld=0, wsb=need - 1) == W
        assert call(r=0) == nat.SKF_OK and call(c=0) == nat.SKF_OK
        bad = C.c_size_t(12345)
        assert lib.skf_fill_unknown_workspace_bytes(-1, cols, C.byref(bad)) == E and bad.value == 12345
        assert lib.skf_fill_unknown_workspace_bytes(rows, cols, None) == E
        # (mask_ld is not looked at without a mask)
        rt.call('skf_fill_unknown', F64, x.ptr, x.ld, rows, cols, None, 0, CONST, 1.5, ws.ptr, need, None)
        np.testing.assert_array_equal(x.download(), np.where(np.isnan(X), 1.5, X))


# ---------------------------------------------------------------------------------------------------------------------------
# skf_cast
# ---------------------------------------------------------------------------------------------------------------------------
CAST_PAIRS = [(F32, F64), (F64, F32), (F32, F32), (F64, F64)]          # (destination, source)


def f32_of_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def cast_specials_f64():
    """Doubles at the seams of the f64 -> f32 rounding: for f32 patterns of both parities (1.0 and its neighbours, the last
    pattern of a binade -- its midpoint rounds up ACROSS the binade --, the largest finite f32 -- its midpoint with 2^128 is
    the overflow threshold --, the subnormals and the step into the normals, 64 random patterns), both signs, the double
    exactly on the midpoint to the next pattern and its two neighbours among the doubles; +-0, +-inf, +-NaN, doubles far
    outside the f32 range on both ends."""
    rs = np.random.RandomState(11)
    pats = np.concatenate([np.array([0x3F800000, 0x3F800001, 0x3F7FFFFF, 0x3FFFFFFF, 0x3FFFFFFE, 0x7F7FFFFF, 0x7F7FFFFE, 0x00000000,
                                     0x00000001, 0x00000002, 0x007FFFFF, 0x007FFFFE, 0x00800000, 0x00400000, 0x00400001], dtype=np.uint32),
                           rs.randint(0x00000001, 0x7F7FFFFF, size=64).astype(np.uint32)])
    lo = f32_of_bits(pats).astype(np.float64)
    hi = np.where(pats == 0x7F7FFFFF, 2.0 ** 128, f32_of_bits(np.minimum(pats + 1, 0x7F7FFFFF)).astype(np.float64))
    mid = lo + (hi - lo) / 2                               # exact: lo and hi are neighbours of 24 bits
    assert (pats & 1).any() and (~pats & 1).any()
    mag = np.concatenate([lo, mid, np.nextafter(mid, 0.0), np.nextafter(mid, np.inf)])
    other = np.array([0.0, np.inf, np.nan, 1e39, 1e300, np.finfo(np.float64).max, 1e-46, 1e-50, 2.0 ** -150, 5e-324, 2.0 ** -1022])
    mag = np.concatenate([mag, other])
    return np.concatenate([mag, -mag])


def cast_specials_f32():
    pats = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3F800001, 0x7F7FFFFF, 0x7F800000, 0x7FC00000,
                     0x33800000, 0x00400000], dtype=np.uint32)
    return f32_of_bits(np.concatenate([pats, pats | np.uint32(0x80000000)]))


def cast_source(src_dtype, rows, cols):
    """The specials first, then randn scaled over 60 binades; repeated to the size of the matrix (a shape of at least 700
    entries holds every special of its type)."""
    rs = np.random.RandomState(seed_of(rows, cols, src_dtype))
    noise = rs.randn(2000) * 2.0 ** rs.randint(-30, 31, size=2000)
    if src_dtype == F64:
        pool = np.concatenate([cast_specials_f64(), noise])
    else:
        pool = np.concatenate([cast_specials_f32(), noise.astype(np.float32)])
    return np.resize(pool, rows * cols).reshape(rows, cols)


def cast_case(shape, dst_dtype, src_dtype):
    rows, cols = shape
    X = cast_source(src_dtype, rows, cols)
    assert X.dtype == NPD[src_dtype]
    with np.errstate(over='ignore'):
        want = X.astype(NPD[dst_dtype])
    with guarded() as g:
        rt = g.rt
        for dpad in (0, 3):
            for spad in (0, 3):
                src = Held(rt.mem, X, cols + spad)
                dst = Held(rt.mem, None, cols + dpad, NPD[dst_dtype], shape)
                rt.call('skf_cast', dst_dtype, dst.ptr, dst.ld, src_dtype, src.ptr, src.ld, rows, cols, None)
                same_values(dst.download(), want, 'cast %s %s -> %s, ldd cols + %d, lds cols + %d'
                            % (shape_id(shape), nat_name(src_dtype), nat_name(dst_dtype), dpad, spad))
                src.unchanged('source')


def cast_specials_are_covered():
    """The shape the specials are judged at holds all of them, and they are what their description says."""
    s = cast_specials_f64()
    assert s.size <= 65 * 97 and cast_specials_f32().size <= 65 * 97
    with np.errstate(over='ignore'):
        f = s.astype(np.float32)
    assert np.isinf(f[np.isfinite(s)]).any()                              # past the overflow threshold
    assert ((f != 0) & (np.abs(f) < 2.0 ** -126)).any()                   # subnormal results
    assert ((f == 0) & (s != 0)).any()                                    # underflow to zero
    assert (np.abs(f) == 2.0).any() and (np.abs(s) < 2.0)[np.abs(f) == 2.0].any()          # up across a binade
    assert (np.abs(f) == np.finfo(np.float32).max).any()


def cast_refusals_case():
    rows, cols = 5, 7
    X = cast_source(F64, rows, cols)
    with guarded() as g:
        rt, lib = g.rt, g.rt.lib
        src = Held(rt.mem, X, cols + 3)
        dst = Held(rt.mem, None, cols + 3, np.float64, (rows, cols))
        E = nat.SKF_E_INVALID

        def call(dd=F32, d=dst.ptr, ldd=dst.ld, sd=F64, s=src.ptr, lds=src.ld, r=rows, c=cols):
            rc = lib.skf_cast(dd, d, ldd, sd, s, lds, r, c, None)
            src.unchanged('source'), dst.unchanged('destination')
            return rc
        assert call(dd=BF16) == E and call(sd=BF16) == E and call(dd=5) == E
        assert call(d=None) == E and call(s=None) == E
        assert call(r=-1) == E and call(c=-1) == E
        assert call(ldd=cols - 1) == E, 'ldd < cols is taken'
        assert call(lds=cols - 1) == E, 'lds < cols is taken'
        assert call(ldd=0) == E and call(lds=-cols) == E
        assert call(ldd=cols, lds=cols, r=0) == nat.SKF_OK and call(c=0) == nat.SKF_OK


# ---------------------------------------------------------------------------------------------------------------------------
# skf_to_bf16
# ---------------------------------------------------------------------------------------------------------------------------
def bf16_rne(u32):
    """Round-to-nearest-even of f32 bit patterns to bf16 bit patterns, stated on the integers: keep the upper 16 bits, go one
    pattern up when the dropped 16 bits are above half, or exactly half with an odd kept pattern (the carry into the exponent
    IS the rounding up across a binade and into infinity).  NaN: the upper 16 bits with the quiet bit set."""
    u = np.asarray(u32).astype(np.uint64)
    keep, rest = u >> np.uint64(16), u & np.uint64(0xFFFF)
    up = (rest > 0x8000) | ((rest == 0x8000) & ((keep & np.uint64(1)) == 1))
    nan = (u & np.uint64(0x7FFFFFFF)) > 0x7F800000
    out = np.where(nan, keep | np.uint64(0x40), keep + up.astype(np.uint64))
    assert (out <= 0xFFFF).all()
    return out.astype(np.uint16)


NAN_PATTERNS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFF8000, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
TABLE_COLS = 509


def rounding_table():
    """f32 bit patterns: for every finite bf16 pattern h -- h itself, the midpoint to its successor, one f32 ulp below and one
    above it --, then +-0, +-inf, the largest finite f32, f32 and bf16 subnormals, and NAN_PATTERNS LAST; zero-filled to a
    matrix of TABLE_COLS columns.  Returns (matrix of uint32, flat indices of the NaN patterns)."""
    h = np.arange(65536, dtype=np.uint32)
    h = h[(h & 0x7F80) != 0x7F80] << 16
    mid = h + np.uint32(0x8000)
    extra = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x007FFFFF,
                      0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x007F8000, 0x807F8000], dtype=np.uint32)
    flat = np.concatenate([h, mid, mid - np.uint32(1), mid + np.uint32(1), extra, NAN_PATTERNS])
    nan_at = np.arange(flat.size - NAN_PATTERNS.size, flat.size)
    rows = -(-flat.size // TABLE_COLS)
    out = np.zeros(rows * TABLE_COLS, dtype=np.uint32)
    out[:flat.size] = flat
    return out.reshape(rows, TABLE_COLS), nan_at


def host_helper_case():
    """nat.to_bf16_bits against bf16_rne on the whole table; the NaN rows are reported apart from the rest."""
    U, nan_at = rounding_table()
    got, want = nat.to_bf16_bits(U.view(np.float32)).reshape(-1), bf16_rne(U).reshape(-1)
    rest = np.ones(got.size, dtype=bool)
    rest[nan_at] = False
    np.testing.assert_array_equal(got[rest], want[rest], err_msg='nat.to_bf16_bits: finite and infinite patterns')
    np.testing.assert_array_equal(got[nan_at], want[nan_at], err_msg='nat.to_bf16_bits: the NaN rows of the rounding table %s'
                                  % ' '.join('%08x' % p for p in NAN_PATTERNS))
    np.testing.assert_array_equal(want[nan_at], [0x7FC0, 0xFFC0, 0x7FC0, 0x7FFF, 0x7FFF, 0xFFFF])
    # f64 input: rounded to f32 first, as the device does
    d = np.array([1.0 + 2.0 ** -8 + 2.0 ** -40, np.nan, -np.inf])
    np.testing.assert_array_equal(nat.to_bf16_bits(d), bf16_rne(d.astype(np.float32).view(np.uint32)))


def run_to_bf16(rt, src_dtype, X, transpose, ldd, spad, zeroed, what):
    """skf_to_bf16 of X (stored as it is) into a destination of leading dimension ldd whose every element holds POISON (or 0:
    `zeroed`) beforehand; returns the result in the orientation of X."""
    rows, cols = X.shape
    src = Held(rt.mem, X, cols + spad)
    dshape = (cols, rows) if transpose else (rows, cols)
    dst = Held(rt.mem, None, ldd, np.uint16, dshape, fill=0 if zeroed else POISON)
    rt.call('skf_to_bf16', dst.ptr, ldd, src_dtype, src.ptr, src.ld, rows, cols, 1 if transpose else 0, None)
    got = dst.download()                                    # (padding: poison stays poison, zero stays zero)
    src.unchanged(what + ': source')
    return got.T if transpose else got


def to_bf16_table_case(src_dtype):
    """f32: the rounding table against bf16_rne, both layouts.  f64: the SPECIFIED behaviour is two roundings, f64 -> f32 ->
    bf16, the same on host and device; the table's values as doubles, and for every midpoint the doubles next to it on either
    side, which the first rounding moves ONTO the midpoint (so the tie rule decides where one rounding from f64 would not
    have seen a tie).  The result is at most 2^-17 ulp (of bf16) from a single rounding: the first rounding moves the value by
    at most half an f32 ulp = 2^-17 bf16 ulp."""
    U, _ = rounding_table()
    if src_dtype == F32:
        X, want = U.view(np.float32), bf16_rne(U)
    else:
        u = U.reshape(-1)
        finite = u[(u & 0x7FFFFFFF) < 0x7F800000]
        mids = finite[(finite & 0xFFFF) == 0x8000].view(np.float32).astype(np.float64)
        quiet = np.array([np.nan, -np.nan, np.inf, -np.inf])
        d = np.concatenate([finite.view(np.float32).astype(np.float64), np.nextafter(mids, np.inf), np.nextafter(mids, -np.inf), quiet])
        rows = -(-d.size // TABLE_COLS)
        X = np.zeros(rows * TABLE_COLS)
        X[:d.size] = d
        X = X.reshape(rows, TABLE_COLS)
        with np.errstate(over='ignore'):
            f = X.astype(np.float32)
        moved = np.nextafter(mids, np.inf).astype(np.float32).astype(np.float64) == mids
        assert moved.all(), 'the first rounding does not move the hair above a midpoint onto it'
        want = bf16_rne(f.view(np.uint32))
    rows, cols = X.shape
    with guarded() as g:
        for transpose in (False, True):
            width = rows if transpose else cols
            got = run_to_bf16(g.rt, src_dtype, X, transpose, width + 3, 3, False, 'table')
            same_bits(got, want, 'to_bf16 rounding table, %s source, %s' % (nat_name(src_dtype), 'transposed' if transpose else 'plain'))


def to_bf16_copy_case():
    """bf16 source: every one of the 65 536 patterns comes back unchanged, NaNs included, in both layouts."""
    X = (np.arange(257 * 256) & 0xFFFF).astype(np.uint16).reshape(257, 256)
    assert np.unique(X).size == 65536
    with guarded() as g:
        for transpose in (False, True):
            width = 257 if transpose else 256
            same_bits(run_to_bf16(g.rt, BF16, X, transpose, width + 3, 3, False, 'copy'), X, 'bf16 -> bf16, transposed %d' % transpose)


def to_bf16_source(src_dtype, rows, cols):
    rs = np.random.RandomState(seed_of(rows, cols, 40 + src_dtype))
    if src_dtype == BF16:
        X = rs.randint(0, 65536, size=(rows, cols)).astype(np.uint16)
        return X, X
    u = rs.randint(0, 2 ** 32, size=(rows, cols), dtype=np.uint64).astype(np.uint32)        # any f32 pattern, NaNs included
    if src_dtype == F32:
        return u.view(np.float32), bf16_rne(u)
    u = np.where((u & 0x7FFFFFFF) > 0x7F800000, (u & np.uint32(0x80000000)) | np.uint32(0x7FC00000), u)      # (NaN: the two default ones)
    X = u.view(np.float32).astype(np.float64) * (1.0 + rs.rand(rows, cols) * 2.0 ** -20)
    with np.errstate(over='ignore', invalid='ignore'):
        return X, bf16_rne(X.astype(np.float32).view(np.uint32))


def to_bf16_layout_case(shape, src_dtype):
    """Both layouts at one shape: ldd = width + 3 over poison, and ldd = the padded width the engine uses (pad64) over zeros,
    which stay zero; lds = cols and cols + 3."""
    rows, cols = shape
    X, want = to_bf16_source(src_dtype, rows, cols)
    with guarded() as g:
        for transpose in (False, True):
            width = rows if transpose else cols
            for ldd, zeroed, spad in ((width + 3, False, 3), (pad64(width), True, 0), (width, False, 3)):
                what = 'to_bf16 %s %s transposed %d ldd %d' % (shape_id(shape), nat_name(src_dtype), transpose, ldd)
                same_bits(run_to_bf16(g.rt, src_dtype, X, transpose, ldd, spad, zeroed, what), want, what)


def to_bf16_refusals_case():
    rows, cols = 5, 3
    X = np.arange(15, dtype=np.float32).reshape(rows, cols)
    with guarded() as g:
        rt, lib = g.rt, g.rt.lib
        src = Held(rt.mem, X, cols + 3)
        dst = Held(rt.mem, None, 8, np.uint16, (rows, 8))               # room for either layout
        E = nat.SKF_E_INVALID

        def call(d=dst.ptr, ldd=8, sd=F32, s=src.ptr, lds=src.ld, r=rows, c=cols, t=0):
            rc = lib.skf_to_bf16(d, ldd, sd, s, lds, r, c, t, None)
            src.unchanged('source'), dst.unchanged('destination')
            return rc
        assert call(sd=3) == E and call(sd=-1) == E, 'a bad source dtype is taken'
        assert call(d=None) == E and call(s=None) == E and call(r=-1) == E and call(c=-1) == E
        assert call(ldd=cols - 1) == E, 'ldd < cols is taken'
        assert call(lds=cols - 1) == E, 'lds < cols is taken'
        assert call(lds=cols - 1, t=1) == E, 'lds < cols is taken (transposed)'
        assert call(ldd=rows - 1, t=1) == E, 'transposed: ldd < rows is taken (ldd >= cols)'
        assert call(ldd=0) == E and call(ldd=-8, t=1) == E
        assert call(r=0) == nat.SKF_OK and call(c=0, t=1) == nat.SKF_OK
        # the least each layout needs is taken: ldd = cols plain, ldd = rows transposed
        rt.call('skf_to_bf16', dst.ptr, cols, F32, src.ptr, src.ld, rows, cols, 0, None)
        rt.call('skf_to_bf16', dst.ptr, rows, F32, src.ptr, src.ld, rows, cols, 1, None)
        got = rt.mem.to_host(dst.buf, (40,), np.uint16)
        same_bits(got[:15].reshape(cols, rows), bf16_rne(X.view(np.uint32)).T, 'ldd = rows, transposed')


def y_extent_case():
    """rows = 2 097 185, cols = 3, f32 source, transposed: 65 537 tiles of 32 rows, a grid whose y extent is past 65 535 (and
    65 536).  The required outcome is the correct result."""
    rows, cols = Y_EXTENT
    rs = np.random.RandomState(9)
    X = (rs.randn(rows, cols) * 2.0 ** rs.randint(-20, 21, size=(rows, cols))).astype(np.float32)
    X[-1] = [1.0 + 2.0 ** -8, -3.0, 2.0 ** -130]
    with guarded() as g:
        got = run_to_bf16(g.rt, F32, X, True, rows + 3, 3, False, 'y extent')
    same_bits(got, bf16_rne(X.view(np.uint32)), 'to_bf16 transposed, %d rows' % rows)


# ---------------------------------------------------------------------------------------------------------------------------
# skf_fill_uniform
# ---------------------------------------------------------------------------------------------------------------------------
def fill_uniform_case(shape=(8209, 67), seed=21, scale=2.5, shift=-0.75):
    """hash_uniform(seed, r * cols + c) * scale + shift with ld = cols + 3 -- the counter runs over cols, not ld -- for f64,
    f32 and bf16, bit for bit.  The generator's values are k / 2^24; with scale 2.5 and shift -0.75 the product and the sum
    are exact in f64, so neither the order of the two operations nor their contraction into one can show: the f64 result is
    THE value, f32 its one rounding, bf16 the rounding of that f32 (bf16_rne)."""
    from oracle.dfmf_oracle import hash_uniform_matrix
    rows, cols = shape
    want = hash_uniform_matrix(seed, rows, cols) * scale + shift
    assert np.array_equal(want, (hash_uniform_matrix(seed, rows, cols) * 2 ** 24 * 5 - 3 * 2 ** 23) / 2 ** 25)
    with guarded() as g:
        rt = g.rt
        for dtype in (F64, F32, BF16):
            for pad in (3, 0):
                dst = Held(rt.mem, None, cols + pad, NPD[dtype], shape)
                rt.call('skf_fill_uniform', dtype, dst.ptr, rows, cols, dst.ld, seed, scale, shift, None)
                got = dst.download()
                expect = bf16_rne(want.astype(np.float32).view(np.uint32)) if dtype == BF16 else want.astype(NPD[dtype])
                same_bits(got, expect, 'fill_uniform %s %s ld cols + %d' % (shape_id(shape), nat_name(dtype), pad))
        dst = Held(rt.mem, None, cols + 3, np.float64, (5, cols))
        assert rt.lib.skf_fill_uniform(F64, dst.ptr, 5, cols, cols - 1, seed, scale, shift, None) == nat.SKF_E_INVALID
        dst.unchanged('refused fill_uniform')
