// skf_gemm_launch.inc -- part of the one translation unit skf_api.hip (textually included there, inside its namespaces; not a
// header of its own): tile choice, split-K models, the ONE slicing decision per product family (slice_gemm, slice_bf16: launches
// and scratch sizing alike) and the launches of the f32 / f64 GEMM kernels and of the bf16 relation contraction.
// ------------------------------------------------------------------------------------------
// GEMM dispatch
// ------------------------------------------------------------------------------------------
struct TileCfg {
    int bm, bn, bk;
};

template <typename T> struct Tiles;
template <> struct Tiles<float> {
    static constexpr int BK = 32;
    static TileCfg big() { return {128, 128, BK}; }
    static TileCfg small() { return {64, 64, BK}; }
};
// f64: a 128 x 128 tile needs 128 accumulator registers + staging = 376 registers (1 wave per
// SIMD); 64 x 128 (2 x 4 MFMA tiles per wave) fits several waves per SIMD
template <> struct Tiles<double> {
    static constexpr int BK = 16;
    static TileCfg big() { return {64, 128, BK}; }
    static TileCfg small() { return {32, 32, BK}; }
    // c x c x c products of the backbone algebra (c <= 512): latency-bound -- many small tiles over
    // the chip and few, deep K steps instead of 8 workgroups walking 16 shallow ones
    static TileCfg deep() { return {32, 32, 64}; }
};
template <typename T> struct BigWave;
template <> struct BigWave<float> { static constexpr int WR = 2, WC = 2; };     // 128 x 128
template <> struct BigWave<double> { static constexpr int WR = 2, WC = 4; };    //  64 x 128

static TileCfg pick_tile(bool is_f64, int engine, int M, int N, int K = 0, bool all_f64 = false) {
    if (engine == SKF_ENGINE_VALU) return {64, 64, 16};
    if (all_f64 && K >= 64 && K <= 1024 && (int64_t)M * N <= 512 * 512) return Tiles<double>::deep();
    const bool big = (M > 64 && N > 64);
    if (is_f64) return big ? Tiles<double>::big() : Tiles<double>::small();
    return big ? Tiles<float>::big() : Tiles<float>::small();
}

// tiles of a symmetric M x M product that touch the lower triangle (GemmArgs::sym)
static int sym_tiles(const TileCfg& t, int M) {
    int n = 0;
    for (int by = 0; by * t.bm < M; ++by) {
        const int cnt = (by * t.bm + t.bm - 1) / t.bn + 1, all = cdiv(M, t.bn);
        n += cnt < all ? cnt : all;
    }
    return n;
}

// number of K slices: fill the chip (>= ~512 workgroups) when the output has few tiles
static int pick_splits(const TileCfg& t, int M, int N, int K, bool sym = false) {
    const int64_t tiles = sym ? sym_tiles(t, M) : (int64_t)cdiv(M, t.bm) * cdiv(N, t.bn);
    if (tiles >= 256) return 1;
    const int ktiles = cdiv(K, t.bk);
    int s = (int)(512 / tiles);
    if (ktiles < 32) return 1;                                   // short contractions (c x c x c) are not split
    const int max_by_k = ktiles / 8 > 0 ? ktiles / 8 : 1;       // at least 8 K tiles per slice
    if (s > max_by_k) s = max_by_k;
    if (s > 256) s = 256;
    return s < 1 ? 1 : s;
}

// K slices for the relation contractions of the f32 / f64 engines (tiles >= 256: pick_splits leaves them unsplit).  Their
// launches are matrix-core bound and their workgroup counts sit just above a multiple of what the chip holds: config 3's
// 50 000-row relations are 782 tiles of 128 x 128 on 768 slots (3 workgroups per CU), the 100 000-row one 1564 -- 14 / 28
// workgroups run a round of their own (a workgroup alone on its CU runs about three times as fast as one of three, so the
// tail costs a third of a round: 75 % efficiency at one round, 86 % at two).  More slices dilute the tail:
//   time(s) = (full rounds + ceil(tail workgroups / 256) / 3) x (K tiles per slice + 4) x step + s x (partial write + read)
// with the step of a workgroup on a full CU (f32 128 x 128 x 32: 6.5 us, f64 64 x 128 x 16: 3.7 us).  Round 5, config 3:
// f32 engine 9.9 -> 11.4 it/s (P12: 5 slices).
static int pick_splits_relation(const TileCfg& t, int M, int N, int K, bool is_f64) {
    const int64_t tiles = (int64_t)cdiv(M, t.bm) * cdiv(N, t.bn);
    const int ktiles = cdiv(K, t.bk);
    const double occ = 3.0, slots = 256.0 * occ, step_us = is_f64 ? 3.7 : 6.5;
    const double slice_us = (double)M * (double)N * (is_f64 ? 8.0 : 4.0) * 2.0 / 4.0e6;      // partials written and re-read at ~4 TB/s
    int best = 1;
    double best_t = 1e300;
    for (int sl = 1; sl <= 16; ++sl) {
        if (sl > 1 && ktiles / sl < 64) break;
        const double wgs = (double)tiles * sl;
        const double full = (double)(int64_t)(wgs / slots), rem = wgs - full * slots;
        const double rounds = full + (rem > 0.0 ? (double)(int64_t)((rem + 255.0) / 256.0) / occ : 0.0);
        const double tt = rounds * (cdiv(ktiles, sl) + 4) * step_us + (sl > 1 ? sl * slice_us : 0.0);
        if (tt < best_t * 0.97) {
            best_t = tt;
            best = sl;
        }
    }
    return best;
}

// operand / result types of one contraction (SKF_F64 or SKF_F32 each).  Supported:
//   (f64,f64,f64)  f64 engine, and the c x c algebra of every engine
//   (f32,f32,f32)  relation contractions and Theta products of the f32 engine
//   (f64,f32,f32)  Gram = G^T G and W = G^T P of the f32 engine: f32 operands, f64 arithmetic
//   (f32,f32,f64)  n x c x c products of the f32 engine with an f64 backbone / B, D matrix
struct GemmTypes {
    int c, a, b;
};

// the staging mode the kernel's stage_mode() would pick for an operand, evaluated on the host (every K slice starts at a
// multiple of k_chunk)
template <typename TS>
static int host_stage_mode(const void* src, int64_t s_row, int64_t s_k, int row_end, int K, int k_chunk) {
    constexpr int V = 16 / (int)sizeof(TS);
    const bool aligned = (((uintptr_t)src) & 15) == 0;
    if (s_k == 1 && aligned && s_row % V == 0 && K % V == 0 && k_chunk % V == 0) return STAGE_VEC_K;
    if (s_row == 1 && aligned && s_k % V == 0 && row_end % V == 0) return STAGE_VEC_R;
    return STAGE_SCALAR;
}

// The big tile stages its operands with COMPILE-TIME modes (with run-time modes the unrolled staging code of both forms
// ran the f32 kernels out of registers: 15 - 57 spilled per lane).  The layouts the engines produce have instantiations:
//   K|R  A along K, B along its rows   P = R G_j, Theta G, H = G_i S, the n x c x c side products
//   R|R  both along their rows         Q = R^T G_i, Gram = G^T G, W = G_i^T P
//   K|K  both along K                  the reconstruction H G_j^T of the f32 / f64 completion and residual
// (every K slice starts at a multiple of the K tile, so the slicing never changes the verdict).  Returns the mode pair, or
// -1: no instantiation -- such a product runs on the small tile, whose run-time modes cost no registers that matter.
constexpr int FM_KR = STAGE_VEC_K | (STAGE_VEC_R << 2), FM_RR = STAGE_VEC_R | (STAGE_VEC_R << 2), FM_KK = STAGE_VEC_K | (STAGE_VEC_K << 2);
static int big_tile_modes(GemmTypes ty, const GemmArgs& g, bool relation) {
    const int bk = (ty.c == SKF_F64) ? Tiles<double>::BK : Tiles<float>::BK;
    const int ma = ty.a == SKF_F64 ? host_stage_mode<double>(g.A, g.sa_m, g.sa_k, g.M, g.K, bk)
                                   : host_stage_mode<float>(g.A, g.sa_m, g.sa_k, g.M, g.K, bk);
    const int mb = ty.b == SKF_F64 ? host_stage_mode<double>(g.B, g.sb_n, g.sb_k, g.N, g.K, bk)
                                   : host_stage_mode<float>(g.B, g.sb_n, g.sb_k, g.N, g.K, bk);
    const int fm = ma | (mb << 2);
    const bool same = ty.a == ty.c && ty.b == ty.c;
    if (same) return (fm == FM_KR || fm == FM_RR || (fm == FM_KK && !relation)) ? fm : -1;
    if (ty.c == SKF_F64) return fm == FM_RR ? fm : -1;           // (f64, f32, f32)
    return fm == FM_KR ? fm : -1;                                // (f32, f32, f64)
}
static bool is_big_tile(const TileCfg& t, bool is_f64) {
    const TileCfg big = is_f64 ? Tiles<double>::big() : Tiles<float>::big();
    return t.bm == big.bm && t.bn == big.bn && t.bk == big.bk;
}
// the tile a product runs on (slice_gemm, and callers that size per-workgroup outputs: skf_relation_sqerr)
static TileCfg gemm_tile(GemmTypes ty, int engine, const GemmArgs& g, bool deep_ok, bool relation) {
    const bool is_f64 = (ty.c == SKF_F64);
    const TileCfg t = pick_tile(is_f64, engine, g.M, g.N, g.K, deep_ok);
    if (engine == SKF_ENGINE_MFMA && is_big_tile(t, is_f64) && big_tile_modes(ty, g, relation) < 0)
        return is_f64 ? Tiles<double>::small() : Tiles<float>::small();
    return t;
}

// How a product is cut into K slices: decided HERE and nowhere else (slice_gemm: f32 / f64 products, slice_bf16: the bf16 contraction),
// for the launches and for the scratch sizing of skf_plan_create alike.  The slice count fixes the summation order, hence the bits.
struct Slicing {
    TileCfg t;
    int splits, k_chunk, sym;       // K slices, K elements per slice, the GemmArgs::sym word of the launch
    bool clamped; int wanted;       // a scratch was given and the `wanted` slices of the MODEL did not fit it
    bool sym_ok;                    // the symmetric model applied (whether or not the launch ends up split)
    size_t part_elems;              // scratch elements the launch is checked against: the slices BEFORE the K-tile rounding (0: one)
};
constexpr int64_t SCRATCH_NONE = -1, SCRATCH_ANY = INT64_MAX;     // `avail`: no scratch at all / as much as the product asks for
// `splits` slices of `per` elements each, clamped to the scratch, then whole K tiles per slice
static void fit_slices(Slicing& d, int splits, size_t per, int K, int want_splits, int64_t avail) {
    if (splits > 1 && (avail < 0 || per * splits > (size_t)avail)) {
        d.clamped = avail >= 0 && want_splits <= 0;
        d.wanted = splits;
        splits = avail >= 0 ? (int)((size_t)avail / per) : 1;
    }
    if (splits < 1) splits = 1;
    d.part_elems = splits > 1 ? per * splits : 0;
    const int ktiles = cdiv(K > 0 ? K : 1, d.t.bk);
    if (splits > ktiles) splits = ktiles;
    d.k_chunk = cdiv(ktiles, splits) * d.t.bk;
    d.splits = cdiv(K > 0 ? K : 1, d.k_chunk);
}
static Slicing slice_gemm_on(const TileCfg& t, GemmTypes ty, int engine, const GemmArgs& g, int want_splits, bool relation, int64_t avail) {
    Slicing d{t, 1, 0, 0, false, 0, false, 0};
    d.sym_ok = g.sym && g.M == g.N && engine == SKF_ENGINE_MFMA && t.bn > t.bm && g.epi == EPI_STORE;
    int splits = want_splits > 0 ? want_splits : pick_splits(t, g.M, g.N, g.K, d.sym_ok);
    if (want_splits <= 0 && relation && engine == SKF_ENGINE_MFMA && g.epi == EPI_STORE && t.bm >= 64 &&
        (int64_t)cdiv(g.M, t.bm) * cdiv(g.N, t.bn) >= 256)
        splits = pick_splits_relation(t, g.M, g.N, g.K, ty.c == SKF_F64);
    if (g.epi == EPI_SQDIFF) splits = 1;
    fit_slices(d, splits, (size_t)g.M * g.N, g.K, want_splits, avail);
    // a symmetric product (the caller says so: Gram = G^T G) computes the tiles on and below the diagonal only; the reduce of
    // the K slices mirrors the rest (GemmArgs::sym).  Unsplit launches write C themselves and compute every tile.
    d.sym = (d.sym_ok && d.splits > 1) ? (t.bm | (t.bn << 16)) : 0;
    return d;
}
static Slicing slice_gemm(GemmTypes ty, int engine, const GemmArgs& g, int want_splits, bool relation, int64_t avail) {
    const bool all_f64 = (ty.c == SKF_F64 && ty.a == SKF_F64 && ty.b == SKF_F64);
    return slice_gemm_on(gemm_tile(ty, engine, g, all_f64 && want_splits <= 1, relation), ty, engine, g, want_splits, relation, avail);
}
// Scratch elements a plan's launch of this product can ask for (`g`: sizes, epilogue, sym flag).  skf_plan_create knows no operand address
// yet, and gemm_tile leaves the big tile when layout or alignment have no big-tile instantiation: the larger of the two outcomes.
static size_t gemm_part_elems(GemmTypes ty, int engine, const GemmArgs& g, bool relation) {
    if (g.M <= 0 || g.N <= 0) return 0;
    const bool is_f64 = (ty.c == SKF_F64);
    const TileCfg t = pick_tile(is_f64, engine, g.M, g.N, g.K, is_f64 && ty.a == SKF_F64 && ty.b == SKF_F64);
    size_t e = slice_gemm_on(t, ty, engine, g, 0, relation, SCRATCH_ANY).part_elems;
    if (engine == SKF_ENGINE_MFMA && is_big_tile(t, is_f64))
        e = std::max(e, slice_gemm_on(is_f64 ? Tiles<double>::small() : Tiles<float>::small(), ty, engine, g, 0, relation, SCRATCH_ANY).part_elems);
    return e;
}

template <typename T, typename TA, typename TB>
static void launch_gemm_t(int engine, const TileCfg& t, GemmArgs g, int splits, bool relation, hipStream_t st) {
    dim3 grid(cdiv(g.N, t.bn), cdiv(g.M, t.bm), splits);
    if (g.sym) grid = dim3((unsigned)sym_tiles(t, g.M), 1, splits);      // (GemmArgs::sym: the tiles on / below the diagonal)
    dim3 block(GEMM_THREADS);
    constexpr int WRB = BigWave<T>::WR, WCB = BigWave<T>::WC;
    const bool big = (t.bm == Tiles<T>::big().bm && t.bn == Tiles<T>::big().bn);
    if (engine == SKF_ENGINE_VALU) {
        hipLaunchKernelGGL((gemm_valu_kernel<T, TA, TB>), grid, block, 0, st, g);
    } else if (t.bk == 64 && t.bm == 32) {         // Tiles<double>::deep()
        if constexpr (std::is_same<T, double>::value && std::is_same<TA, double>::value &&
                      std::is_same<TB, double>::value)
            hipLaunchKernelGGL((gemm_mfma_kernel<double, double, double, 1, 1, 64, 0>), grid, block, 0, st, g);
        else
            SKF_FAIL(SKF_E_INVALID, "deep tile is f64 only");
    } else if (big) {
        constexpr int BKT = Tiles<T>::BK;
        constexpr bool same = std::is_same<TA, T>::value && std::is_same<TB, T>::value;
        const int fm = big_tile_modes(GemmTypes{std::is_same<T, double>::value ? SKF_F64 : SKF_F32, std::is_same<TA, double>::value ? SKF_F64 : SKF_F32,
                                                std::is_same<TB, double>::value ? SKF_F64 : SKF_F32}, g, relation);
        if (fm < 0) SKF_FAIL(SKF_E_INVALID, "big tile without a staging layout (gemm_tile picks the small tile for these)");
#define SKF_BIG(TAG_, FM_) hipLaunchKernelGGL((gemm_mfma_kernel<T, TA, TB, WRB, WCB, BKT, TAG_, FM_>), grid, block, 0, st, g)
        if constexpr (same) {
            if (relation) {
                if (fm == FM_KR) SKF_BIG(1, FM_KR);
                else SKF_BIG(1, FM_RR);
            } else {
                if (fm == FM_KR) SKF_BIG(0, FM_KR);
                else if (fm == FM_RR) SKF_BIG(0, FM_RR);
                else SKF_BIG(0, FM_KK);
            }
        } else if constexpr (std::is_same<T, double>::value) {      // (f64, f32, f32): Gram = G^T G and W = G_i^T P of the f32 / bf16 engines
            SKF_BIG(0, FM_RR);
        } else {                                                     // (f32, f32, f64): n x c x c products with an f64 backbone
            SKF_BIG(0, FM_KR);
        }
#undef SKF_BIG
    } else {
        hipLaunchKernelGGL((gemm_mfma_kernel<T, TA, TB, 1, 1, Tiles<T>::BK, 0>), grid, block, 0, st, g);
    }
    check_launch("gemm");
    if (splits > 1) {
        if (splits >= 8)
            hipLaunchKernelGGL((splitk_reduce_z16_kernel<T>), dim3(elem_grid((int64_t)g.M * g.N * 16)), dim3(256), 0, st,
                               g, splits);
        else
            hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3(elem_grid((int64_t)g.M * g.N)), dim3(256), 0, st,
                               g, splits);
        check_launch("splitk_reduce");
    }
}

// `part`/`part_bytes`: scratch for split-K partials; the slices are clamped to fit (slice_gemm), and a clamped model is counted.
static void run_gemm(GemmTypes ty, int engine, GemmArgs g, int want_splits, void* part, size_t part_bytes,
                     hipStream_t st, bool relation = false) {
    if (g.M <= 0 || g.N <= 0) return;
    const int64_t avail = part ? (int64_t)(part_bytes / (ty.c == SKF_F64 ? 8 : 4)) : SCRATCH_NONE;
    const Slicing d = slice_gemm(ty, engine, g, want_splits, relation, avail);
    if (d.clamped) {
        ++g_split_clamps;
        if (env_int("SKF_DEBUG_CLAMP", 0))
            fprintf(stderr, "skf: split-K clamp, gemm %dx%dx%d types %d/%d/%d tile %dx%d relation %d sym %d: %d slices wanted, scratch holds %zu\n",
                    g.M, g.N, g.K, ty.c, ty.a, ty.b, d.t.bm, d.t.bn, (int)relation, (int)d.sym_ok, d.wanted, (size_t)avail / ((size_t)g.M * g.N));
    }
    g.k_chunk = d.k_chunk;
    g.part = part;
    g.sym = d.sym;
    if (ty.c == SKF_F64 && ty.a == SKF_F64 && ty.b == SKF_F64)
        launch_gemm_t<double, double, double>(engine, d.t, g, d.splits, relation, st);
    else if (ty.c == SKF_F32 && ty.a == SKF_F32 && ty.b == SKF_F32)
        launch_gemm_t<float, float, float>(engine, d.t, g, d.splits, relation, st);
    else if (ty.c == SKF_F64 && ty.a == SKF_F32 && ty.b == SKF_F32)
        launch_gemm_t<double, float, float>(engine, d.t, g, d.splits, relation, st);
    else if (ty.c == SKF_F32 && ty.a == SKF_F32 && ty.b == SKF_F64)
        launch_gemm_t<float, float, double>(engine, d.t, g, d.splits, relation, st);
    else
        SKF_FAIL(SKF_E_INVALID, "unsupported operand type combination (c=%d a=%d b=%d)", ty.c, ty.a, ty.b);
}

// Two independent all-f64 products of the c x c chains in ONE launch (gemm_mfma_pair_kernel) when both take the deep
// unsplit tile of the matrix-core engine -- what run_gemm picks for them one by one; anything else: two launches.
static void run_gemm_pair_f64(int engine, GemmArgs a, GemmArgs b, hipStream_t st, bool allow) {
    const GemmTypes ty{SKF_F64, SKF_F64, SKF_F64};
    auto deep = [&](const GemmArgs& g) {            // deep tile, one slice?
        if (engine != SKF_ENGINE_MFMA || g.M <= 0 || g.N <= 0 || g.sym || g.epi == EPI_SQDIFF) return false;
        const Slicing d = slice_gemm(ty, engine, g, 0, false, SCRATCH_ANY);
        return d.t.bk == 64 && d.t.bm == 32 && d.splits == 1;
    };
    if (!allow || !deep(a) || !deep(b)) {
        run_gemm(ty, engine, a, 0, nullptr, 0, st);
        run_gemm(ty, engine, b, 0, nullptr, 0, st);
        return;
    }
    const TileCfg t = Tiles<double>::deep();
    for (GemmArgs* g : {&a, &b}) {                  // (as run_gemm sets an unsplit launch up)
        g->k_chunk = slice_gemm(ty, engine, *g, 0, false, SCRATCH_ANY).k_chunk;
        g->part = nullptr;
    }
    const int gx = std::max(cdiv(a.N, t.bn), cdiv(b.N, t.bn)), gy = std::max(cdiv(a.M, t.bm), cdiv(b.M, t.bm));
    hipLaunchKernelGGL((gemm_mfma_pair_kernel<double, double, double, 1, 1, 64, 0>), dim3(gx, gy, 2), dim3(GEMM_THREADS), 0, st, a, b);
    check_launch("gemm_pair");
}

// The symmetric split-K products G^T G of several types in ONE product launch and ONE reduce launch (gemm_mfma_group_kernel,
// round 6) when every one of them is what run_gemm would launch as a big-tile symmetric split with at least 8 slices and the
// scratch holds all their slices side by side; returns false otherwise (the caller then issues them one by one).  Tile,
// slices, K chunk and sym word per product come from slice_gemm, as run_gemm's do: the results are the same bits.
template <typename TM>
static bool run_gram_group_t(int engine, const GemmArgs* gs, int n, void* part, size_t part_bytes, hipStream_t st) {
    constexpr bool m64 = std::is_same<TM, double>::value;
    const GemmTypes ty{SKF_F64, m64 ? SKF_F64 : SKF_F32, m64 ? SKF_F64 : SKF_F32};
    if (engine != SKF_ENGINE_MFMA || n < 2 || n > 4 || part == nullptr) return false;
    GemmGroup m;
    memset(&m, 0, sizeof m);
    size_t off = 0;                      // f64 elements of the scratch handed out so far
    int max_tiles = 0, max_splits = 0;
    int64_t max_elems = 0;
    for (int i = 0; i < n; ++i) {
        GemmArgs g = gs[i];
        if (g.M <= 0 || g.M != g.N || !g.sym || g.epi != EPI_STORE || g.gate != nullptr) return false;
        // what the group saves is two launch boundaries per product; a product of several GFLOP runs for 0.1 ms and more and
        // loses that to sharing its rounds with the others (same box, config 3: 1/10 scale +5.3 %, 1/5 +2.2 %, full size -0.7 %)
        if (2.0 * (double)g.K * (double)g.M * (double)g.N > 4.0e9) return false;
        const Slicing d = slice_gemm(ty, engine, g, 0, false, SCRATCH_ANY);
        if (!is_big_tile(d.t, true) || big_tile_modes(ty, g, false) != FM_RR) return false;
        if (d.splits < 8) return false;                                  // (the many-slice reduce; a small type: nothing to gain)
        const size_t slices = (size_t)g.M * g.N * d.splits;
        if ((off + slices) * 8 > part_bytes) return false;
        g.part = (double*)part + off;
        off += slices;
        g.k_chunk = d.k_chunk;
        g.sym = d.sym;
        m.g[i] = g;
        m.tiles[i] = sym_tiles(d.t, g.M);
        m.splits[i] = d.splits;
        max_tiles = std::max(max_tiles, m.tiles[i]);
        max_splits = std::max(max_splits, d.splits);
        max_elems = std::max(max_elems, (int64_t)g.M * g.N);
    }
    constexpr int WRB = BigWave<double>::WR, WCB = BigWave<double>::WC, BKT = Tiles<double>::BK;
    hipLaunchKernelGGL((gemm_mfma_group_kernel<double, TM, TM, WRB, WCB, BKT, 0, FM_RR>), dim3(max_tiles, n, max_splits),
                       dim3(GEMM_THREADS), 0, st, m);
    check_launch("gemm_group");
    hipLaunchKernelGGL((splitk_reduce_z16_group_kernel<double>), dim3(elem_grid(max_elems * 16), n), dim3(256), 0, st, m);
    check_launch("splitk_reduce_group");
    return true;
}

// ---- bf16 relation contraction --------------------------------------------------------------
static inline int64_t pad64(int64_t v) { return (v + 63) / 64 * 64; }

// K slices for the bf16 contraction.  Time model of a launch (microseconds): the workgroups run in
// ceil(units * s / slots) rounds of (K tiles per slice + 3 tiles of prologue / epilogue) x 1.5 us, and s > 1 slices
// write and re-read s partial copies of the output at ~3 TB/s.  On config 3 it picks what the A/B runs of rounds 1 / 2
// picked (5 / 3 / 3 / 3 slices for P12 / Q12 / P23 / Q23); a product with a handful of output tiles (config 5,
// genre x movie: ONE 256 x 256 tile over K = 40000, 0.96 ms in one workgroup before) is cut into up to 64 slices.
static int pick_splits_bf16(int64_t units, int ktiles, int bm, int64_t out_elems) {
    const double cus = 256.0;                                       // resident workgroups: one (256 rows) or two per CU
    const double slots = cus * (bm >= 256 ? 1.0 : 2.0);
    const double per_slice_us = (double)out_elems * 8.0 / 3.0e6;
    int best = 1;
    double best_t = 1e300;
    for (int s = 1; s <= 64; ++s) {
        if (s > 1 && ktiles / s < 4) break;
        const double rounds = (double)(int64_t)((double)units * s / slots + 0.999999);
        const double t = (rounds < 1.0 ? 1.0 : rounds) * ((ktiles + s - 1) / s + 3) * 1.5 + (s > 1 ? s * per_slice_us : 0.0);
        // more slices only for a clear gain (HBM-bound launches have none).  Round 3, profiles/r03_split_margin.txt: with the
        // margin at 1.0 the model cuts P13 (196 of 256 CUs busy, one slice) into five slices -- inside the iteration that
        // launch then takes 1.23 ms instead of 1.19 and the fit loses 0.7 %: the 60 idle CUs are not idle, the side
        // products of the second stream run there.
        if (t < best_t * 0.97) {
            best_t = t;
            best = s;
        }
    }
    return best;
}

// rows per workgroup of the bf16 contraction: the 256-row LDS-DMA kernel for large problems and for
// every transposed-A product, the 128-row register-staged kernel for small P-type products
static int bf16_block_rows(int M, bool at) { return (at || M >= 4096) ? 256 : 128; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and DEVICE (the attribute belongs to the kernel's
// code object on one device: a process that drives several GPUs sets it on each), safe against the concurrent host
// threads of run_fits_concurrent (one plan per thread)
constexpr int SKF_MAX_DEVICES = 64;
constexpr int SKF_MAX_BATCH = 64;        // plans of one skf_iterate_batch call
struct DeviceOnce {
    std::once_flag flag[SKF_MAX_DEVICES];
};
template <class K>
static void allow_dynamic_lds(DeviceOnce& once, K kernel, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SKF_MAX_DEVICES) dev = 0;
    hipError_t err = hipSuccess;
    std::call_once(once.flag[dev], [&] { err = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
    if (err != hipSuccess) SKF_FAIL(SKF_E_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(err));
}

// the bf16 contraction (rows256: a transposed or bitmap A operand -- always the 256-row kernel; `avail` in f32 elements)
static Slicing slice_bf16(int M, int N, int Kp, bool rows256, int want_splits, int64_t avail) {
    Slicing d{{bf16_block_rows(M, rows256), (N <= 128) ? 128 : 256, 64}, 1, 0, 0, false, 0, false, 0};
    const int splits = want_splits > 0 ? want_splits
                                       : pick_splits_bf16((int64_t)cdiv(M, d.t.bm) * cdiv(N, d.t.bn), Kp / 64, d.t.bm, (int64_t)M * N);
    fit_slices(d, splits, (size_t)M * N, Kp, want_splits, avail);
    return d;
}
static size_t bf16_part_bytes(int M, int N, int Kp, bool rows256) {
    return slice_bf16(M, N, Kp, rows256, 0, SCRATCH_ANY).part_elems * sizeof(float);
}

// C[M x N] (f32) = op(A) * Bt^T, bf16 operands:  at == false: A is [M][lda] (K contiguous);
// at == true: A is [Kp][lda] row-major with the OUTPUT rows along its columns (lda >= M, rows zero-padded to Kp)
static void run_gemm_bf16(const uint16_t* A, int64_t lda, const uint16_t* Bt, int64_t ldb, float* C, int64_t ldc,
                          int M, int N, int Kp, int want_splits, void* part, size_t part_bytes, bool relation,
                          hipStream_t st, bool at = false, bool abits = false) {
    if (M <= 0 || N <= 0) return;
    // abits: A is the bitmap of a binary relation, lda its row pitch in bytes (8 entries per byte)
    const int64_t a_cols = abits ? lda * 8 : lda;
    if (Kp % 64 != 0 || lda % 8 != 0 || ldb % 8 != 0 || (!at && a_cols < Kp) || (at && a_cols < M) || ldb < Kp)
        SKF_FAIL(SKF_E_INVALID, "bf16 contraction: inner dimension must be padded to 64 (Kp=%d lda=%lld ldb=%lld)", Kp,
                 (long long)lda, (long long)ldb);
    if ((((uintptr_t)A) | ((uintptr_t)Bt)) & 15) SKF_FAIL(SKF_E_INVALID, "bf16 operands must be 16-byte aligned");
    const Slicing d = slice_bf16(M, N, Kp, at || abits, want_splits, part ? (int64_t)(part_bytes / sizeof(float)) : SCRATCH_NONE);
    if (d.clamped) {
        ++g_split_clamps;
        if (env_int("SKF_DEBUG_CLAMP", 0))
            fprintf(stderr, "skf: split-K clamp, bf16 contraction %dx%dx%d at %d bits %d: %d slices wanted, scratch holds %zu\n", M, N, Kp,
                    (int)at, (int)abits, d.wanted, part_bytes / sizeof(float) / ((size_t)M * N));
    }
    const int bm = d.t.bm, bn = d.t.bn, splits = d.splits;
    Bf16GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = A; g.Bt = Bt; g.C = C; g.part = (float*)part;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.M = M; g.N = N; g.Kp = Kp;
    g.a_kstep = 64; g.b_kstep = 64;
    g.k_chunk = d.k_chunk;
    dim3 grid(cdiv(N, bn), cdiv(M, bm), splits);
    if (bm == 256) {
        // 256 x BN tile, LDS rings in dynamic shared memory (> 64 KiB needs the attribute)
        // (SKF_V2_POLICY: what the K loop does -- the product's V2Full unless a bound-finding build of tools/probe names
        // a policy of its own on the command line, the way SKF_A_AUX names the cache policy)
#ifndef SKF_V2_POLICY
#define SKF_V2_POLICY V2Full
#endif
#define SKF_V2_LAUNCH(BN_, TAG_, AT_)                                                                             \
    do {                                                                                                          \
        const int smem_ = (3 * 256 + ((BN_ == 256) ? 2 : 3) * BN_) * 8 * 16;                                      \
        static DeviceOnce once_;                                                                              \
        allow_dynamic_lds(once_, gemm_bf16_v2_kernel<BN_, TAG_, AT_, EPI_T_STORE, false, SKF_V2_POLICY>, smem_);  \
        hipLaunchKernelGGL((gemm_bf16_v2_kernel<BN_, TAG_, AT_, EPI_T_STORE, false, SKF_V2_POLICY>), grid, dim3(512), smem_, st, g); \
    } while (0)
#define SKF_V2_LAUNCH_BITS(BN_, AT_)                                                                              \
    do {                                                                                                          \
        const int smem_ = (3 * 256 + ((BN_ == 256) ? 2 : 3) * BN_) * 8 * 16;                                      \
        static DeviceOnce once_;                                                                              \
        allow_dynamic_lds(once_, gemm_bf16_v2_kernel<BN_, 1, AT_, EPI_T_STORE, true>, smem_);                     \
        hipLaunchKernelGGL((gemm_bf16_v2_kernel<BN_, 1, AT_, EPI_T_STORE, true>), grid, dim3(512), smem_, st, g); \
    } while (0)
        if (abits) {
            if (at && bn == 128) SKF_V2_LAUNCH_BITS(128, true);
            else if (at) SKF_V2_LAUNCH_BITS(256, true);
            else if (bn == 128) SKF_V2_LAUNCH_BITS(128, false);
            else SKF_V2_LAUNCH_BITS(256, false);
        } else if (at) {
            if (bn == 128) SKF_V2_LAUNCH(128, 1, true);
            else SKF_V2_LAUNCH(256, 1, true);
        } else if (bn == 128 && relation) SKF_V2_LAUNCH(128, 1, false);
        else if (bn == 128) SKF_V2_LAUNCH(128, 0, false);
        else if (relation) SKF_V2_LAUNCH(256, 1, false);
        else SKF_V2_LAUNCH(256, 0, false);
#undef SKF_V2_LAUNCH
#undef SKF_V2_LAUNCH_BITS
    } else {
        dim3 block(256);
        if (bn == 128) hipLaunchKernelGGL((gemm_bf16_kernel<128, 0>), grid, block, (128 + 128) * 128, st, g);
        else hipLaunchKernelGGL((gemm_bf16_kernel<256, 0>), grid, block, (128 + 256) * 128, st, g);
    }
    check_launch("gemm_bf16");
    if (splits > 1) {
        hipLaunchKernelGGL(bf16_splitk_reduce_kernel, dim3(elem_grid(((int64_t)M * N + 3) / 4)), dim3(256), 0, st, C, ldc,
                           (const float*)part, M, N, splits);
        check_launch("bf16_splitk_reduce");
    }
}

template <typename TS>
static void launch_to_bf16(uint16_t* dst, int64_t ldd, const TS* src, int64_t lds, int64_t rows, int64_t cols,
                           bool transpose, hipStream_t st) {
    if (rows <= 0 || cols <= 0) return;
    if (transpose) {
        dim3 grid((unsigned)cdiv(cols, 32), (unsigned)cdiv(rows, 32));
        hipLaunchKernelGGL((transpose_to_bf16_kernel<TS>), grid, dim3(256), 0, st, dst, ldd, src, lds, rows, cols);
    } else {
        hipLaunchKernelGGL((to_bf16_kernel<TS>), dim3(elem_grid(rows * cols)), dim3(256), 0, st, dst, ldd, src, lds,
                           rows, cols);
    }
    check_launch("to_bf16");
}
