"""What DevicePlan's constructor tells the library, for every kind of input it accepts: the descriptors that reach
skf_plan_create (per relation row_type, col_type, row_begin, n_rows, flags, known_bound, ld, mask_ld and whether data / mask
are null; per constraint type, ld, nnz and whether data is null; every field of the options) and the names, subjects and
order of the skf_plan_set_* calls that follow -- read off Runtime.call on the host emulator -- and every refusal of the
constructor by exception type and full text.  The expectations are written from include/skfusion_hip.h and the
constructor's docstring, not taken from a run."""
import numpy as np
import pytest

from emul.runtime import emulated_runtime, use_runtime

import skfusion_amd._native as nat
from skfusion_amd._engine import (DevicePlan, DeviceMatrix, KnownEntries, PackedMask, owned_rows, pack_mask,
                                  upload_known_entries, upload_matrix)

ABSENT, NO_COL, MASKED, BITS, BINARY = (nat.SKF_REL_ABSENT, nat.SKF_REL_NO_COL_SIDE, nat.SKF_REL_MASKED,
                                        nat.SKF_REL_MASK_BITS, nat.SKF_REL_BINARY)
LISTS, KNOWN, SPARSE, FOLD, RANK1 = (nat.SKF_REL_KNOWN_LISTS, nat.SKF_REL_KNOWN_CSR, nat.SKF_REL_SPARSE_CSR,
                                     nat.SKF_REL_FOLD_CSR, nat.SKF_REL_FILL_RANK1)
F64, F32, BF16 = nat.SKF_F64, nat.SKF_F32, nat.SKF_BF16
DFMF, DFMC, TRANSFORM = nat.SKF_DFMF, nat.SKF_DFMC, nat.SKF_TRANSFORM
MFMA, VALU = nat.SKF_ENGINE_MFMA, nat.SKF_ENGINE_VALU
OWNED, THETA_OWNED = nat.SKF_OPT_OWNED_ROWS, nat.SKF_OPT_THETA_OWNED_ROWS

TYPES = ['a', 'b', 'c']
N = {'a': 40, 'b': 30, 'c': 20}
RANK = {'a': 4, 'b': 3, 'c': 8}
N64 = {'a': 128, 'b': 64, 'c': 64}          # bf16: the ownership chunk and the row blocks are multiples of 64


@pytest.fixture(scope='module', autouse=True)
def emul():
    with use_runtime(emulated_runtime()) as rt:
        yield rt


def described(monkeypatch, *args, **kwargs):
    """DevicePlan(*args, **kwargs) -> (relations, constraints, options, set calls) as the library was told."""
    rt = nat.get_runtime()
    real, seen = rt.call, {'sets': []}

    def call(fname, *a):
        if fname == 'skf_plan_create':
            n_types, _, n_rel, rdesc, n_theta, hdesc, opt, _ = a
            seen['types'] = n_types
            seen['rels'] = [(r.row_type, r.col_type, r.row_begin, r.n_rows, r.flags, r.known_bound, r.ld, r.mask_ld,
                             r.data is None, r.mask is None) for r in (rdesc[k] for k in range(n_rel))]
            seen['thetas'] = [(h.type, h.ld, h.nnz, h.data is None) for h in (hdesc[k] for k in range(n_theta))]
            o = opt._obj
            seen['opt'] = (o.dtype, o.variant, o.target_type, o.engine, o.part_index, o.part_count, o.flags)
        elif fname.startswith('skf_plan_set_'):
            seen['sets'].append((fname[len('skf_plan_set_'):], a[1]))
        return real(fname, *a)
    monkeypatch.setattr(rt, 'call', call)
    plan = DevicePlan(*args, **kwargs)
    try:
        assert seen['types'] == len(args[0])
        return seen['rels'], seen['thetas'], seen['opt'], seen['sets'], plan
    finally:
        monkeypatch.undo()
        plan.close()


def rel(row, col, flags=0, known=0, ld=0, mask_ld=0, begin=0, rows=0, data=True, mask=False):
    """One expected relation descriptor: (row_type, col_type, row_begin, n_rows, flags, known_bound, ld, mask_ld, data is
    NULL, mask is NULL)."""
    return (row, col, begin, rows, flags, known, ld, mask_ld, not data, not mask)


def opts(dtype=F64, variant=DFMF, target=-1, engine=MFMA, part=(0, 0), flags=0):
    return (dtype, variant, target, engine, part[0], part[1], flags)


def matrices(seed=0, n=N):
    rs = np.random.RandomState(seed)
    return rs.rand(n['a'], n['b']), rs.rand(n['a'], n['c'])


def mask_of(shape, seed=1):
    return np.random.RandomState(seed).rand(*shape) < 0.3          # True = unknown


def entries(shape, unstored, seed=2, by_col=False, fill=False, density=0.2):
    """KnownEntries of a random pattern (every line holds an entry or not, as it falls)."""
    import scipy.sparse
    rs = np.random.RandomState(seed)
    dense = np.where(rs.rand(*shape) < density, rs.rand(*shape) + 0.5, 0.0)
    sp = scipy.sparse.csc_matrix(dense) if by_col else scipy.sparse.csr_matrix(dense)
    sp.sort_indices()
    kw = dict(row_fill=np.full(shape[0], 0.25), col_fill=np.ones(shape[1])) if fill else {}
    return KnownEntries(sp.indptr, sp.indices, sp.data, shape, unstored=unstored, by_col=by_col, **kw)


# ---- dense relations, host and device, the three mask forms -----------------------------------------------------------------
@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('mask_form', [None, 'host', 'packed', 'bytes'])
def test_dense_relations_and_their_masks(where, mask_form, monkeypatch):
    rt = nat.get_runtime()
    Rab, Rac = matrices()
    data = upload_matrix(Rab, 'f64', rt) if where == 'device' else Rab
    m = mask_of(Rab.shape)
    known = int(m.size - np.count_nonzero(m))
    if mask_form == 'host':
        mask, want = m, dict(flags=BITS, known=known, mask_ld=4, mask=True)             # 30 columns: 4 bytes of bits a row
    elif mask_form == 'packed':
        mask, want = pack_mask(m, rt.mem), dict(flags=BITS, known=known, mask_ld=4, mask=True)
        assert isinstance(mask, PackedMask)
    elif mask_form == 'bytes':
        mask = DeviceMatrix(rt.mem.from_host(m.astype(np.uint8)), m.shape)
        mask.known = known
        want = dict(flags=0, known=known, mask_ld=30, mask=True)
    else:
        mask, want = None, {}
    rels, thetas, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, [('a', 'b', data, mask), ('a', 'c', Rac, None)], [],
                                              DFMC)
    assert rels == [rel(0, 1, ld=30, **want), rel(0, 2, ld=20)]
    assert thetas == [] and sets == [] and opt == opts(variant=DFMC)
    assert plan.local_rows == [40, 40] and plan.theta_rows == [] and plan.rel_over_fill == {} and plan.owned is False


def test_sparse_known_false_drops_the_bound_of_every_mask_form(monkeypatch):
    rt = nat.get_runtime()
    Rab, Rac = matrices()
    m = mask_of(Rab.shape)
    byte_mask = DeviceMatrix(rt.mem.from_host(mask_of(Rac.shape).astype(np.uint8)), Rac.shape)
    byte_mask.known = 7
    rels, _, opt, sets, _ = described(monkeypatch, TYPES, N, RANK, [('a', 'b', Rab, m), ('a', 'c', Rac, byte_mask),
                                                                     ('b', 'c', np.ones((30, 20)), pack_mask(mask_of((30, 20)), rt.mem))],
                                      [], DFMC, sparse_known=False, engine=VALU)
    assert rels == [rel(0, 1, BITS, 0, 30, 4, mask=True), rel(0, 2, 0, 0, 20, 20, mask=True), rel(1, 2, BITS, 0, 20, 3, mask=True)]
    assert sets == [] and opt == opts(variant=DFMC, engine=VALU)


# ---- 0 / 1 relations under bf16 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('verdict', [None, True, False])
def test_binary_relations_under_bf16(verdict, monkeypatch):
    """A host 0 / 1 array is found binary; a block's `binary` verdict replaces the look at the data, either way; a mask or
    another dtype never is; a DeviceMatrix is as binary as it says."""
    rt = nat.get_runtime()
    rs = np.random.RandomState(3)
    Z = (rs.rand(N64['a'], N64['b']) < 0.5).astype(np.float64)
    if verdict is None:
        relations, kw = [('a', 'b', Z, None)], {}
        want = rel(0, 1, BINARY, ld=64)
    else:
        blk = dict(row_begin=64, n_rows=64, absent=False, col_side=True, masked=False, binary=verdict)
        relations, kw = [('a', 'b', Z[64:] + (0.0 if verdict else 0.5), None, blk)], dict(part=(1, 2))
        want = rel(0, 1, BINARY if verdict else 0, ld=64, begin=64, rows=64)
    # (the second relation: real-valued, so that the plan is not all bitmaps)
    relations.append(('a', 'c', rs.rand(N64['a'], N64['c'])[:64 if verdict is not None else None], None) +
                     ((dict(row_begin=64, n_rows=64, binary=False),) if verdict is not None else ()))
    rels, _, opt, sets, plan = described(monkeypatch, TYPES, N64, RANK, relations, [], DFMF, dtype='bf16', **kw)
    more = dict(begin=64, rows=64) if verdict is not None else {}
    assert rels == [want, rel(0, 2, ld=64, **more)]
    assert sets == [] and opt == opts(dtype=BF16, part=kw.get('part', (0, 0)))
    assert plan.local_rows == ([64, 64] if verdict is not None else [128, 128])


def test_binary_takes_bf16_and_no_mask(monkeypatch):
    rt = nat.get_runtime()
    Z = (np.random.RandomState(3).rand(N64['a'], N64['b']) < 0.5).astype(np.float64)
    dev = DeviceMatrix(rt.mem.from_host(nat.to_bf16_bits(Z)), Z.shape, binary=True)
    plain = DeviceMatrix(rt.mem.from_host(nat.to_bf16_bits(Z)), Z.shape)
    rels, _, _, _, _ = described(monkeypatch, TYPES[:2], N64, RANK, [('a', 'b', dev, None), ('a', 'b', plain, None),
                                                                     ('a', 'b', Z, mask_of(Z.shape)), ('a', 'b', dev, mask_of(Z.shape))],
                                 [], DFMC, dtype='bf16')
    known = int(Z.size - np.count_nonzero(mask_of(Z.shape)))
    assert rels == [rel(0, 1, BINARY, ld=64), rel(0, 1, ld=64), rel(0, 1, BITS, known, 64, 8, mask=True),
                    rel(0, 1, BITS, known, 64, 8, mask=True)]
    rels, _, opt, _, _ = described(monkeypatch, TYPES[:2], N64, RANK, [('a', 'b', Z, None)], [], DFMF, dtype='f32')
    assert rels == [rel(0, 1, ld=64)] and opt == opts(dtype=F32)


# ---- row blocks ---------------------------------------------------------------------------------------------------------------
def test_row_blocks_present_absent_and_without_column_side(monkeypatch):
    """Rank 1 of 2 of a row-block fit: the second half of (a, b) with its column side, the first rows of (a, c) without it,
    nothing of (b, c)."""
    Rab, Rac = matrices()
    relations = [('a', 'b', Rab[20:], None, dict(row_begin=20, n_rows=20, absent=False, col_side=True, masked=False)),
                 ('a', 'c', Rac[:8], None, dict(row_begin=0, n_rows=8, col_side=False)),
                 ('b', 'c', None, None, dict(row_begin=0, n_rows=0, absent=True, col_side=False, masked=False))]
    rels, _, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, relations, [], DFMF, part=(1, 2))
    assert rels == [rel(0, 1, ld=30, begin=20, rows=20), rel(0, 2, NO_COL, ld=20, rows=8),
                    rel(1, 2, ABSENT | NO_COL, data=False)]
    assert sets == [] and opt == opts(part=(1, 2))
    assert plan.local_rows == [20, 8, 0] and plan.owned is False


@pytest.mark.parametrize('known_lists', [False, True])
def test_masked_row_blocks_and_the_known_lists_verdict(known_lists, monkeypatch):
    """A masked block keeps the bound of its mask only where the caller decided for lists (`known_lists`, owned rows); an
    absent block of a masked relation carries the same flags and no data."""
    Rab, Rac = matrices()
    m = mask_of(Rab.shape)[:20]
    known = int(m.size - np.count_nonzero(m))
    assert owned_rows('f64', 40, 0, 2)[:2] == (0, 20) and owned_rows('f64', 30, 0, 2)[:2] == (0, 15)
    relations = [('a', 'b', Rab[:20], m, dict(row_begin=0, n_rows=20, absent=False, masked=True, known_lists=known_lists)),
                 ('a', 'c', Rac[:20], None, dict(row_begin=0, n_rows=20, masked=False))]
    rels, _, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, relations, [], DFMC, part=(0, 2), owned=True)
    assert rels == [rel(0, 1, MASKED | BITS | (LISTS if known_lists else 0), known if known_lists else 0, 30, 4, rows=20, mask=True),
                    rel(0, 2, ld=20, rows=20)]
    assert sets == [] and opt == opts(variant=DFMC, part=(0, 2), flags=OWNED)
    assert plan.local_rows == [20, 20] and plan.owned is True
    # bf16, 40 objects: rank 1 of 2 owns no row of 'a' (the chunk is 64-aligned) -- the absent form of the same relations
    assert owned_rows('bf16', 40, 1, 2)[:2] == (40, 0)
    relations = [('a', 'b', None, None, dict(row_begin=0, n_rows=0, absent=True, masked=True, known_lists=known_lists)),
                 ('a', 'c', None, None, dict(row_begin=0, n_rows=0, absent=True))]
    rels, _, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, relations, [], DFMC, dtype='bf16', part=(1, 2), owned=True)
    assert rels == [rel(0, 1, ABSENT | MASKED | (LISTS if known_lists else 0), data=False), rel(0, 2, ABSENT, data=False)]
    assert sets == [] and opt == opts(dtype=BF16, variant=DFMC, part=(1, 2), flags=OWNED) and plan.local_rows == [0, 0]


# ---- relations given as their entries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['unknown', 'zero', 'filled'])
@pytest.mark.parametrize('uploaded', [False, True])
def test_relations_given_as_their_entries(form, uploaded, monkeypatch):
    rt = nat.get_runtime()
    ke = entries((40, 30), 'zero' if form == 'filled' else form, fill=form == 'filled')
    if form == 'unknown':
        ke.fill = 0.75
    data = upload_known_entries(ke, 'f64', rt.mem) if uploaded else ke
    variant = DFMC if form == 'unknown' else DFMF
    rels, _, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, [('a', 'c', matrices()[1], None), ('a', 'b', data, None)], [],
                                         variant)
    flags = {'unknown': KNOWN, 'zero': SPARSE, 'filled': SPARSE | RANK1}[form]
    assert rels == [rel(0, 2, ld=20), rel(0, 1, flags, ke.known, data=False)]
    assert sets == [('known_entries', 1)] + ([('relation_fill', 1)] if form == 'filled' else [])
    assert opt == opts(variant=variant)
    assert plan.rel_over_fill == {'unknown': {1: 0.75}, 'zero': {}, 'filled': {1: None}}[form] and plan.local_rows == [40, 40]


@pytest.mark.parametrize('form', ['unknown', 'zero'])
def test_entries_of_the_owned_rows(form, monkeypatch):
    """Rank 1 of 2: the CSR of rows 20 .. 39 of (a, b) and of rows 15 .. 29 of (b, c), indptr from 0."""
    variant = DFMC if form == 'unknown' else DFMF
    kab, kbc = entries((40, 30), form), entries((30, 20), form, seed=5)
    assert owned_rows('f64', 40, 1, 2)[:2] == (20, 20) and owned_rows('f64', 30, 1, 2)[:2] == (15, 15)
    sab, sbc = kab.row_slice(20, 20), kbc.row_slice(15, 15)
    relations = [('a', 'b', sab, None, dict(row_begin=20, n_rows=20, absent=False, col_side=True, masked=False, entries=form)),
                 ('b', 'c', sbc, None, dict(row_begin=15, n_rows=15, entries=form))]
    rels, _, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, relations, [], variant, part=(1, 2), owned=True)
    flag = KNOWN if form == 'unknown' else SPARSE
    assert rels == [rel(0, 1, flag, sab.known, begin=20, rows=20, data=False), rel(1, 2, flag, sbc.known, begin=15, rows=15, data=False)]
    assert sets == [('known_entries', 0), ('known_entries', 1)] and opt == opts(variant=variant, part=(1, 2), flags=OWNED)
    assert plan.local_rows == [20, 15] and plan.rel_over_fill == ({0: 0.0, 1: 0.0} if form == 'unknown' else {})


@pytest.mark.parametrize('form', ['unknown', 'zero'])
def test_an_absent_block_of_entries(form, monkeypatch):
    """bf16, 40 objects, rank 1 of 2 owns no row of 'a': only the flags of the kind, no lists, nothing uploaded."""
    variant = DFMC if form == 'unknown' else DFMF
    relations = [('a', 'b', None, None, dict(row_begin=0, n_rows=0, absent=True, col_side=True, masked=False, entries=form))]
    rels, _, opt, sets, plan = described(monkeypatch, TYPES[:2], N, RANK, relations, [], variant, dtype='bf16', part=(1, 2), owned=True)
    assert rels == [rel(0, 1, ABSENT | (KNOWN if form == 'unknown' else SPARSE), data=False)]
    assert sets == [] and opt == opts(dtype=BF16, variant=variant, part=(1, 2), flags=OWNED)
    assert plan.local_rows == [0] and plan.rel_over_fill == {} and plan._keep_rel == []


@pytest.mark.parametrize('by_col', [False, True])
def test_fold_in_entries_compressed_along_the_target(by_col, monkeypatch):
    """New objects of 'a' (9 of them): the target is the row type of (a, b) -- row lists -- or the column type of (b, a) --
    column lists.  The dense new relation beside it keeps its plain descriptor."""
    n = {'a': 9, 'b': 30, 'c': 20}
    types = ['a', 'b', 'c']
    if by_col:
        ke, pair = entries((30, 9), 'zero', by_col=True), ('b', 'a')
    else:
        ke, pair = entries((9, 30), 'zero'), ('a', 'b')
    relations = [pair + (ke, None), ('a', 'c', np.random.RandomState(0).rand(9, 20), None)]
    rels, _, opt, sets, plan = described(monkeypatch, types, n, RANK, relations, [], TRANSFORM, target='a')
    assert rels == [rel(1 if by_col else 0, 0 if by_col else 1, FOLD, ke.known, data=False), rel(0, 2, ld=20)]
    assert sets == [('known_entries', 0)] and opt == opts(variant=TRANSFORM, target=0)
    assert plan.rel_over_fill == {} and plan.local_rows == [30 if by_col else 9, 9]


# ---- constraints --------------------------------------------------------------------------------------------------------------
def constraint(n, per_row, seed=4):
    th = np.zeros((n, n))
    rs = np.random.RandomState(seed)
    for r in range(n):
        th[r, rs.choice(n, per_row, replace=False)] = rs.rand(per_row) + 0.1
    return th


def test_dense_constraints_host_and_device(monkeypatch):
    """nnz: the count itself up to n * n / 16 (the library's divisor), 0 = dense beyond it or where nobody counted."""
    rt = nat.get_runtime()
    sparse_a, dense_b = constraint(40, 2), constraint(30, 10)        # 80 <= 1600 / 16 = 100; 300 > 900 / 16
    dev_sparse = upload_matrix(constraint(20, 1), 'f64', rt)
    dev_sparse.nnz = 20                                               # 20 <= 400 / 16 = 25
    dev_uncounted = upload_matrix(constraint(20, 1, seed=6), 'f64', rt)
    dev_dense = upload_matrix(constraint(40, 3), 'f64', rt)
    dev_dense.nnz = 120
    thetas_in = [('a', sparse_a), ('b', dense_b), ('c', dev_sparse), ('c', dev_uncounted), ('a', dev_dense)]
    rels, thetas, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, [('a', 'b', matrices()[0], None), ('a', 'c', matrices()[1], None)],
                                              thetas_in, DFMF)
    assert thetas == [(0, 40, 80, False), (1, 30, 0, False), (2, 20, 20, False), (2, 20, 0, False), (0, 40, 0, False)]
    assert sets == [] and opt == opts() and plan.theta_rows == [40, 30, 20, 20, 40]
    assert rels == [rel(0, 1, ld=30), rel(0, 2, ld=20)]


@pytest.mark.parametrize('uploaded', [False, True])
def test_constraints_given_as_their_entries(uploaded, monkeypatch):
    rt = nat.get_runtime()
    ka, kc = entries((40, 40), 'zero', seed=7, density=0.05), entries((20, 20), 'zero', seed=8, density=0.05)
    give = (lambda k: upload_known_entries(k, 'f64', rt.mem)) if uploaded else (lambda k: k)
    rels, thetas, opt, sets, plan = described(monkeypatch, TYPES, N, RANK,
                                              [('a', 'b', entries((40, 30), 'zero'), None), ('a', 'c', matrices()[1], None)],
                                              [('a', give(ka)), ('b', np.eye(30)), ('c', give(kc))], DFMF)
    assert thetas == [(0, 0, ka.known, True), (1, 30, 30, False), (2, 0, kc.known, True)]
    # the relations' lists are handed over first, then the constraints', each kind in its own order
    assert sets == [('known_entries', 0), ('constraint_entries', 0), ('constraint_entries', 2)]
    assert opt == opts() and plan.theta_rows == [40, 30, 20]


def test_constraint_entries_of_the_owned_rows(monkeypatch):
    """Rank 1 of 2: the slice of rows 20 .. 39 of the constraint on 'a' over all 40 columns; a dense constraint beside it stays
    whole.  The options say that the slices are the owned rows."""
    Rab, Rac = matrices()
    ka = entries((40, 40), 'zero', seed=7, density=0.05)
    sl = ka.row_slice(20, 20)
    relations = [('a', 'b', Rab[20:], None, dict(row_begin=20, n_rows=20)), ('a', 'c', Rac[20:], None, dict(row_begin=20, n_rows=20))]
    rels, thetas, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, relations, [('a', sl), ('b', np.eye(30))], DFMF,
                                              part=(1, 2), owned=True)
    assert thetas == [(0, 0, sl.known, True), (1, 30, 30, False)]
    assert sets == [('constraint_entries', 0)] and opt == opts(part=(1, 2), flags=OWNED | THETA_OWNED)
    assert plan.theta_rows == [20, 30] and plan.local_rows == [20, 20]
    # without entries among the constraints the second flag stays off
    _, thetas, opt, sets, plan = described(monkeypatch, TYPES, N, RANK, relations, [('b', np.eye(30))], DFMF, part=(1, 2), owned=True)
    assert thetas == [(1, 30, 30, False)] and sets == [] and opt == opts(part=(1, 2), flags=OWNED) and plan.theta_rows == [30]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refused(text, *args, **kwargs):
    with pytest.raises(ValueError) as err:
        DevicePlan(*args, **kwargs).close()
    assert type(err.value) is ValueError and str(err.value) == text


def test_every_refusal_of_the_constructor():
    rt = nat.get_runtime()
    Rab, Rac = matrices()
    two = TYPES[:2]
    refused("unsupported engine dtype 7", two, N, RANK, [('a', 'b', Rab, None)], [], DFMF, dtype=7)
    # entries
    blk = dict(row_begin=0, n_rows=0, absent=True, entries='zero')
    refused('relation (a,b): known entries take a row block under row ownership only', two, N, RANK, [('a', 'b', None, None, blk)], [],
            DFMF, part=(1, 2))
    ke = entries((40, 30), 'zero')
    refused('relation (a,b): known entries take no mask and no row block', two, N, RANK, [('a', 'b', ke, mask_of((40, 30)))], [], DFMF)
    refused('relation (a,b): known entries take no mask and no row block', two, N, RANK,
            [('a', 'b', ke.row_slice(0, 20), None, dict(row_begin=0, n_rows=20))], [], DFMF, part=(0, 2))
    refused('relation (a,b) dimension mismatch: (20, 30) vs object counts (40,30)', two, N, RANK, [('a', 'b', ke.row_slice(0, 20), None)],
            [], DFMF)
    refused('relation (a,b) dimension mismatch: (40, 30) vs object counts (20,30)', two, N, RANK,
            [('a', 'b', ke, None, dict(row_begin=0, n_rows=20))], [], DFMF, part=(0, 2), owned=True)
    n9 = {'a': 9, 'b': 30}
    refused('relation (a,b): a filled relation with missing values is for fits, not fold-ins', two, n9, RANK,
            [('a', 'b', entries((9, 30), 'zero', fill=True), None)], [], TRANSFORM, target='a')
    refused('relation (b,a): a fold-in takes the lists compressed along the target a', ['a', 'b'], n9, RANK,
            [('b', 'a', entries((30, 9), 'zero'), None)], [], TRANSFORM, target='a')
    refused('relation (a,b): a fold-in takes the lists compressed along the target a', two, n9, RANK,
            [('a', 'b', entries((9, 30), 'zero', by_col=True), None)], [], TRANSFORM, target='a')
    refused('relation (a,b): lists compressed along the column type are for fold-ins', two, N, RANK,
            [('a', 'b', entries((40, 30), 'zero', by_col=True), None)], [], DFMF)
    # dense
    refused('relation 0 is not a matrix', two, N, RANK, [('a', 'b', np.zeros(40), None)], [], DFMF)
    refused('relation (a,b) dimension mismatch: (40, 20) vs object counts (40,30)', two, N, RANK, [('a', 'b', Rac, None)], [], DFMF)
    refused('relation (a,b) dimension mismatch: (40, 20) vs object counts (40,30)', two, N, RANK,
            [('a', 'b', upload_matrix(Rac, 'f64', rt), None)], [], DFMF)
    refused('relation (a,b) dimension mismatch: (40, 30) vs object counts (20,30)', two, N, RANK,
            [('a', 'b', Rab, None, dict(row_begin=0, n_rows=20))], [], DFMF, part=(0, 2))
    # masks, the three forms
    wrong = mask_of((40, 20))
    byte_mask = DeviceMatrix(rt.mem.from_host(wrong.astype(np.uint8)), wrong.shape)
    for m in (wrong, pack_mask(wrong, rt.mem), byte_mask):
        refused('mask shape mismatch for relation (a,b)', two, N, RANK, [('a', 'b', Rab, m)], [], DFMC)
    refused('mask is not a matrix', two, N, RANK, [('a', 'b', Rab, np.zeros(40, dtype=bool))], [], DFMC)
    # constraints
    rels = [('a', 'b', Rab, None)]
    refused("constraint on a: entries need unstored='zero', compressed along the rows", two, N, RANK, rels,
            [('a', entries((40, 40), 'unknown'))], DFMF)
    refused("constraint on a: entries need unstored='zero', compressed along the rows", two, N, RANK, rels,
            [('a', entries((40, 40), 'zero', by_col=True))], DFMF)
    refused('constraint on a dimension mismatch: (30, 30) vs (40,40)', two, N, RANK, rels, [('a', entries((30, 30), 'zero'))], DFMF)
    refused('constraint on a dimension mismatch: (40, 40) vs (20,40)', two, N, RANK,
            [('a', 'b', Rab[:20], None, dict(row_begin=0, n_rows=20))], [('a', entries((40, 40), 'zero'))], DFMF, part=(0, 2), owned=True)
    refused('constraint on a dimension mismatch', two, N, RANK, rels, [('a', np.eye(30))], DFMF)
    refused('constraint on a dimension mismatch', two, N, RANK, rels, [('a', upload_matrix(np.eye(30), 'f64', rt))], DFMF)


def test_invalid_entries_are_refused_before_any_upload(monkeypatch):
    """upload_known_entries validates on the host: DataFusionError, and the library is never called."""
    from skfusion_amd.fusion import DataFusionError
    rt = nat.get_runtime()
    ke = entries((40, 30), 'zero')
    ke.indices = ke.indices[::-1].copy()
    monkeypatch.setattr(rt, 'call', lambda *a: pytest.fail('the library was called'))
    with pytest.raises(DataFusionError) as err:
        DevicePlan(TYPES[:2], N, RANK, [('a', 'b', ke, None)], [], DFMF)
    assert str(err.value) == 'known entries: columns not strictly ascending within a row (canonical CSR)'
