"""The kernel paths only large inputs reach, at the smallest shapes that reach them, each against a plain reference of the same
operation: the LDS lookups of the evaluation loop (k_lookup_lds: XCD renumbering, the pipelined loop of whole blocks, ragged
channel groups, both mixed dispatches), the rank GEMM with several word tiles per workgroup (k_rank_gemm: accumulator reset,
prefetch across tiles, the clamped last range, the k seam of the last chunk), and the grid-capped reductions and scans of
vbq_reduce.hip (k_moments_flat's main loop, k_moments_bc at its channel limit, k_rd_sums, k_index_max, k_check_inputs) and
vbq_hist.hip (k_hist_tiled with several row passes).

The launchers size their grids from the CU count and from thresholds, so the shapes are derived from the device's CU count with
the launch rules restated in tests/launch_plans.py (kept equal to the sources by tests/test_launch_plans_host.py), and every test
asserts, BEFORE it launches, that its shape takes the path it is named after: on a device whose CU count defeats a shape the
test fails with that message instead of passing through another path."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import launch_plans as LP  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import vbq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _reaches(cond, cus, what):
    if not cond:
        pytest.fail(f"with {cus} CUs this shape does not reach the path under test: {what} (move the shape, tests/launch_plans.py)")


# ================================================================================================ A. lookups out of the LDS
def _bits(t):
    """The tensor's elements as integers of the same width (exact comparison, -0.0 != 0.0)."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        first = tuple(int(v) for v in bad[0])
        pytest.fail(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at [l, row, channel] = {first}: "
                    f"got {got[first].item()!r}, want {want[first].item()!r}")


def _lookup_inputs(L, C, B, N, seed):
    """Rank indices [L, C, B] (u16 planes) uniform over [0, T) with 0, T - 1 and the foreign 65535 planted at the corners of
    the row range, a sorted table, per-lambda length and model tables -- all made on the device."""
    T = 2 ** (N + 1) - 1
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randint(0, T, (L, C, B), device="cuda", generator=g, dtype=torch.int32)
    for l, c in ((0, 0), (L - 1, C - 1), (L // 2, C // 2)):
        q[l, c, :3] = torch.tensor([0, T - 1, 65535], dtype=torch.int32)
        q[l, c, B - 3:] = torch.tensor([65535, 0, T - 1], dtype=torch.int32)
    idx = q.to(torch.int16).view(torch.uint16)                       # 65535 -> -1 -> 0xffff
    srt = torch.sort(torch.randn((C, T), device="cuda", generator=g), dim=1).values.contiguous()
    ll = torch.rand((L, C, N + 1), device="cuda", generator=g) * 20
    models = torch.rand((L, C, T), device="cuda", generator=g) * 14.5 + 0.5
    return q, idx, srt, ll, models


def _check_lookups(L, C, B, N, seed):
    """ops.gather_latents in its three dispatches -- everything asked for, the outputs of the LDS passes alone, the outputs
    of the generic kernel alone -- against torch fancy indexing of the same tables, every element, exactly."""
    from vbq_amd import ops
    T = 2 ** (N + 1) - 1
    q, idx, srt, ll, models = _lookup_inputs(L, C, B, N, seed)
    # the kernels run first, and their results stay alive: no reference value exists yet that a skipped store could inherit
    # from recycled memory
    z, raw_f, nb, qi = ops.gather_latents(idx, N=N, table_sorted=srt, level_len=ll, models=models, want_num_bits=True, want_idx=True)
    z2, none_raw, nb2, none_qi = ops.gather_latents(idx, N=N, table_sorted=srt, models=models, want_raw_bits=False, want_num_bits=True)
    none_z, raw_i, none_nb, qi2 = ops.gather_latents(idx, N=N, want_zhat=False, want_idx=True)
    assert none_raw is None and none_qi is None and none_z is None and none_nb is None
    assert raw_f.dtype == torch.float32 and raw_i.dtype == torch.int32 and qi.dtype == torch.uint16
    qc = q.clamp(max=T - 1).long()                                   # foreign indices >= T stay inside the tables
    lev = torch.from_numpy(O.levels_of_sorted_ranks(N)).cuda()[qc]   # int32 [L, C, B]
    want_z = srt.unsqueeze(0).expand(L, C, T).gather(2, qc).transpose(1, 2).contiguous()
    _same(z, want_z, "Z_hat")
    _same(z2, want_z, "Z_hat (asked for with num_bits alone)")
    del want_z
    want_nb = models.gather(2, qc).transpose(1, 2).contiguous()
    _same(nb, want_nb, "num_bits")
    _same(nb2, want_nb, "num_bits (asked for with Z_hat alone)")
    del want_nb
    _same(raw_f, ll.gather(2, lev.long()).transpose(1, 2).contiguous(), "raw_num_bits (corrected lengths, f32)")
    _same(raw_i, lev.transpose(1, 2).contiguous(), "raw_num_bits (levels, int32)")
    want_qi = qc.to(torch.int16).transpose(1, 2).contiguous()
    _same(qi, want_qi, "channel-last indices")
    _same(qi2, want_qi, "channel-last indices (generic kernel alone)")


def _lookup_shape(cus, C, N, blocks_per_split, last_rows, prefer):
    found = LP.find_lookup_shape(cus, C, N, blocks_per_split, last_rows, prefer=prefer)
    _reaches(found is not None, cus, f"no row count gives C = {C} splits of {blocks_per_split} blocks within 44 M elements")
    return found


@pytest.mark.parametrize("N", [10, 7])
def test_lookup_lds_renumbered_groups_one_pipelined_iteration_then_a_rest_block(cus, N):
    """C = 256 (16 channel groups: the XCD renumbering), splits of three blocks -- one iteration of the pipelined loop, then one
    block of the rest loop -- and a last split of four rows; the num_bits pass walks the whole row range per workgroup.
    256 CUs: L = 8, B = 20 740, 28 splits of 768 rows.  N = 7: another table size beside the tiles in the LDS."""
    C = 256
    L, B = _lookup_shape(cus, C, N, 3, 4, 20740)
    p = LP.lookup_plan(L, C, B, N, cus)
    _reaches(p.z_lds and p.nb_lds and p.renumbered and p.groups % 16 == 0, cus, f"{p}")
    _reaches(LP.walk(p.per) == LP.Walk(1, 1, LP.LDS_ROWS) and p.last_split_rows == 4 and p.splits >= 2, cus, f"{p}")
    _reaches(LP.walk(B).pipelined >= 2 and LP.walk(B).last_rows == 4, cus, f"num_bits pass {LP.walk(B)}")
    _check_lookups(L, C, B, N, seed=100 + N)


def test_lookup_lds_two_pipelined_iterations_per_split(cus):
    """Splits of five blocks: two iterations of the pipelined loop (the index ring refilled from rows the second iteration
    reads), one rest block, the tile flip carried over five blocks and over the lambdas.  256 CUs: L = 5, B = 33 028."""
    C, N = 256, 10
    L, B = _lookup_shape(cus, C, N, 5, None, 33028)
    p = LP.lookup_plan(L, C, B, N, cus)
    _reaches(p.z_lds and p.renumbered and LP.walk(p.per) == LP.Walk(2, 1, LP.LDS_ROWS) and L >= 2, cus, f"{p}")
    _check_lookups(L, C, B, N, seed=2)


def test_lookup_lds_last_group_of_four_channels_over_several_blocks(cus):
    """C = 260: 17 channel groups (no renumbering), the last one holding four channels -- its workgroups take every block
    through the guarded (not FULL) form, three blocks per split.  256 CUs: L = 8, B = 20 740."""
    C, N = 260, 10
    L, B = _lookup_shape(cus, C, N, 3, 4, 20740)
    p = LP.lookup_plan(L, C, B, N, cus)
    _reaches(p.z_lds and p.nb_lds and not p.renumbered and p.last_group_channels == 4, cus, f"{p}")
    _reaches(LP.walk(p.per, whole_group=False) == LP.Walk(0, 3, LP.LDS_ROWS) and p.last_split_rows == 4, cus, f"{p}")
    _check_lookups(L, C, B, N, seed=3)


def test_lookup_lds_many_splits_of_few_groups(cus):
    """C = 64: four channel groups, so the rows split many ways; the last split is one whole block and four rows.
    256 CUs: L = 3, B = 65 540, 86 splits of 768 rows, the last of 260."""
    C, N = 64, 10
    L, B = _lookup_shape(cus, C, N, 3, 260, 65540)
    p = LP.lookup_plan(L, C, B, N, cus)
    _reaches(p.z_lds and p.nb_lds and not p.renumbered and p.splits > p.groups, cus, f"{p}")
    _reaches(LP.walk(p.per) == LP.Walk(1, 1, LP.LDS_ROWS) and LP.walk(p.last_split_rows) == LP.Walk(0, 2, 4), cus, f"{p}")
    _check_lookups(L, C, B, N, seed=4)


def test_lookup_mixed_dispatch_zhat_from_lds_num_bits_generic(cus):
    """L = 64, C = 16, B = 2308: enough lookups per table for Z_hat out of the LDS, too few rows for num_bits, which stays with
    the generic kernel together with raw_num_bits and the indices."""
    L, C, B, N = 64, 16, 2308, 10
    p = LP.lookup_plan(L, C, B, N, cus)
    _reaches(p.z_lds and not p.nb_lds, cus, f"{p}")
    _check_lookups(L, C, B, N, seed=5)


def test_lookup_mixed_dispatch_num_bits_from_lds_zhat_generic(cus):
    """C = 256, B = 3076, L = 2: num_bits out of the LDS (renumbered groups, the pipelined loop over all rows), Z_hat generic."""
    L, C, B, N = 2, 256, 3076, 10
    p = LP.lookup_plan(L, C, B, N, cus)
    _reaches(not p.z_lds and p.nb_lds and p.renumbered and LP.walk(B).pipelined >= 2, cus, f"{p}")
    _check_lookups(L, C, B, N, seed=6)


def test_compress_latents_at_the_model_width_equals_oracle(cus):
    """vbq_compress_latents_f32 at C = 256, B = 3076 (two Kodak images and four rows) with 16 lambdas, corrected lengths and
    entropy models -- planes, solve, num_bits out of the LDS, the rest generic -- against the C oracle's solve plus table
    lookups, every element."""
    from scipy.stats import norm

    from vbq_amd import ops
    N, C, B = 10, 256, 3076
    T = 2 ** (N + 1) - 1
    lam = [float(v) for v in 2.0 ** np.linspace(-8, 7.5, 16)]
    p = LP.lookup_plan(len(lam), C, B, N, cus)
    _reaches(p.nb_lds and not p.z_lds and p.renumbered, cus, f"{p}")
    rng = np.random.default_rng(7)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C))
    xi = np.concatenate([(np.arange(2 ** n) + 0.5) / 2 ** n for n in range(N + 1)])
    tab = norm.ppf(xi[None], scale=scale[:, None]).astype(np.float32)            # level-major [C, T]
    srt = np.empty_like(tab)
    srt[:, O.level_major_to_rank(N)] = tab                                       # the same code points by rank
    assert np.all(np.diff(srt, axis=1) > 0)
    mu = (scale * rng.standard_normal((B, C))).astype(np.float32)
    sg = np.clip(np.exp(-2 + 0.7 * rng.standard_normal((B, C))), 1e-4, 10).astype(np.float32)
    ll = (np.arange(N + 1, dtype=np.float32) + np.abs(rng.normal(0, 1, (len(lam), C, N + 1)))).astype(np.float32)
    models = rng.uniform(0.5, 15, (len(lam), C, T)).astype(np.float32)
    z, raw, nb = ops.compress_latents(torch.from_numpy(mu).cuda(), torch.from_numpy(sg).cuda(), torch.from_numpy(tab).cuda(),
                                      torch.from_numpy(srt).cuda(), lam, N=N, level_len=torch.from_numpy(ll).cuda(),
                                      models=torch.from_numpy(models).cuda())
    wi, wz, wb = CO.quantize(mu, sg, tab, lam, N=N, level_len=ll, want_zhat=True, want_bits=True, threads=8)
    assert np.array_equal(z.cpu().numpy(), wz), "Z_hat differs from the oracle"
    assert np.array_equal(raw.cpu().numpy(), wb), "raw_num_bits differs from the oracle"
    want_nb = models[np.arange(len(lam))[:, None, None], np.arange(C)[None, None, :], wi.astype(np.int64)]
    assert np.array_equal(nb.cpu().numpy(), want_nb), "num_bits differs from models[l, c, oracle index]"
    assert len(np.unique(wi)) > 500                                              # the sweep does use the table


# ================================================================================================ B. rank GEMM
def _rank_inputs(V, K, Q, plan, seed):
    """An embedding and analogy questions with exact score ties planted where a tile mix-up would break them: copies of three
    ground-truth words in the same tile, in the other tile of the same workgroup, in another workgroup's range and in the last
    (partial) tile; a zero row as a question's ground truth and as one of its terms; a question with a = b = c = d."""
    rng = np.random.default_rng(seed)
    if K == 1:
        # one dimension: normed = e / (1e-8 + |e|) is +-1 for every |e| >> 1e-8, all scores tie; magnitudes around 1e-8 spread them
        emb = (rng.choice([-1.0, 1.0], (V, K)) * 10.0 ** rng.uniform(-8.5, -6.5, (V, K))).astype(np.float32)
    else:
        emb = rng.normal(0, 1, (V, K)).astype(np.float32)
    an = rng.integers(0, V, (Q, 4)).astype(np.int32)
    tpw, nt = plan.tiles_per_wg, plan.nt
    bn = LP.RANK_BN
    first_of_last_tile = (nt - 1) * bn
    assert V - first_of_last_tile >= 8 and nt >= tpw + 2
    other_wg = min(2 * tpw, nt - 2)

    def word(tile, off):
        return tile * bn + off

    truths = (word(0, 5), word(tpw + 1, 60), V - 3)                  # first tile of wg 0, second tile of wg 1, last partial tile
    copies = ((word(0, 77), word(1, 9), word(tpw, 3), V - 1),
              (word(tpw + 1, 61), word(tpw, 100), word(0, 101), V - 2),
              (V - 4, word(other_wg, 7), word(other_wg + 1 if other_wg + 1 < nt - 1 else 1, 8), first_of_last_tile))
    for i, (d, cp) in enumerate(zip(truths, copies)):
        emb[list(cp)] = emb[d]
        an[4 * i:4 * i + 3, 3] = d                                   # three questions ask for the word itself ...
        an[4 * i + 3, 3] = cp[1]                                     # ... one for its copy in another tile
    zero = word(1, 50)
    emb[zero] = 0.0                                                  # 0 / 1e-8
    an[12, 3] = zero
    an[13, 1] = zero
    an[14] = word(tpw, 40)                                           # a = b = c = d
    an[Q - 1] = an[0]                                                # the last question of the ragged question block
    planted = sorted({*truths, *[w for cp in copies for w in cp], zero})
    assert len(planted) == 16 and planted[-1] == V - 1
    return emb, an


def _check_ranks(V, K, Q, plan, seed):
    from vbq_amd import embeddings as E
    emb, an = _rank_inputs(V, K, Q, plan, seed)
    got = E.prediction_ranks(torch.from_numpy(emb).cuda(), an).cpu().numpy()
    want = CO.analogy_ranks(emb, an, threads=8)                      # the documented arithmetic: fma chain over ascending k
    differ = np.flatnonzero(got != want)
    assert differ.size == 0, (f"{differ.size} of {Q} ranks differ from the fma-chain checker, first question {differ[0]}: "
                              f"got {got[differ[0]]}, want {want[differ[0]]}")
    r64, near = O.prediction_ranks(emb, an)                          # the notebook's arithmetic in float64
    assert np.all(near[:12] >= 4)                                    # the planted ties are ties
    assert np.all(np.abs(got - r64) <= near), "a rank is further from the float64 rank than the near-ties allow"
    assert got.min() >= 0 and got.max() <= V - 1 and len(np.unique(got)) > Q // 4


@pytest.mark.parametrize("K", [1, 31, 32, 33, 64, 65])
def test_rank_gemm_two_tiles_per_workgroup_and_a_shorter_last_range(cus, K):
    """Every workgroup multiplies two word tiles (accumulators reset at the second, its first stage prefetched during the last
    stage of the first), the last workgroup's range is clamped to one; K on both sides of the 32-wide k-chunk and of its
    even-k seam.  256 CUs: V = 10 277, Q = 1000 -- 81 tiles, 41 workgroups per question block."""
    Q = 1000
    V = LP.find_rank_words(cus, Q, 65, 2, True, prefer=10277)
    _reaches(V is not None, cus, "no vocabulary with V * Q * K <= 1e9 gives two tiles per workgroup and a shorter last range")
    p = LP.rank_plan(V, K, Q, cus)
    _reaches(p.tiles_per_wg >= 2 and p.splits >= 2 and 1 <= p.last_wg_tiles < p.tiles_per_wg and V % LP.RANK_BN and Q % LP.RANK_BM,
             cus, f"{p}")
    assert (p.nk, p.kend_last) == {1: (1, 2), 31: (1, 32), 32: (1, 32), 33: (2, 2), 64: (2, 32), 65: (3, 2)}[K]
    _check_ranks(V, K, Q, p, seed=K)


def test_rank_gemm_three_tiles_per_workgroup(cus):
    """At least three tiles per workgroup: a tile that is neither the first nor the last of its range.  256 CUs: V = 33 000,
    Q = 520, K = 1 -- 258 tiles, 86 workgroups of three."""
    Q, K = 520, 1
    V = LP.find_rank_words(cus, Q, K, 3, False, prefer=33000)
    _reaches(V is not None, cus, "no vocabulary with V * Q * K <= 1e9 gives three tiles per workgroup")
    p = LP.rank_plan(V, K, Q, cus)
    _reaches(p.tiles_per_wg >= 3 and p.splits >= 2 and V % LP.RANK_BN and Q % LP.RANK_BM, cus, f"{p}")
    _check_ranks(V, K, Q, p, seed=303)


# ================================================================================================ C. reductions and scans
def _exact(a):
    """float64 values summed along the last axis without a rounding that matters: np.longdouble where it is wider than
    double (x86: 64-bit mantissa, pairwise), math.fsum otherwise -> float64."""
    a = np.asarray(a)
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        return np.asarray(a.astype(np.longdouble).sum(axis=-1), dtype=np.float64)
    return np.asarray([math.fsum(r) for r in a.reshape(-1, a.shape[-1])]).reshape(a.shape[:-1])


def _check_moments(got, x_cn):
    """got [C, 2] against the exact sums of x_cn [C, n] (f32).  The terms x and x * x are exact in f64 (24- and 48-bit
    significands), so a sum of n of them in ANY order is within n * 2^-53 * sum|t| of the exact one (to first order; the
    factor 2 covers the higher orders and the rounding of the reference to f64)."""
    x = x_cn.astype(np.float64)
    n = x.shape[1]
    for k, t in enumerate((x, x * x)):
        want = _exact(t)
        tol = 2.0 * n * 2.0 ** -53 * _exact(np.abs(t))
        err = np.abs(got[:, k] - want)
        c = int(np.argmax(err - tol))
        assert np.all(err <= tol), f"moment {k + 1} of channel {c}: {got[c, k]!r} against {want[c]!r}, |err| {err[c]:.3e} > {tol[c]:.3e}"


def test_moments_flat_main_loop_one_channel():
    """C = 1 with just enough elements that half of the lanes run one iteration of the main loop (four 16-byte loads in
    flight), the rest only the single-load loop; n % 4 == 3 leaves a scalar tail."""
    from vbq_amd import ops
    gx, need = LP.moments_flat_grid(8_000_000, 1)
    nq = need + gx * LP.THREADS // 2
    n = 4 * nq + 3
    assert LP.moments_flat_grid(n, 1) == (gx, need) and n // 4 > need and n // 4 < need + gx * LP.THREADS
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(n, dtype=np.float32) * np.float32(1.5) + np.float32(0.3))
    got = ops.moments(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (1, 2)
    _check_moments(got, x[None])


@pytest.mark.parametrize("extra", [0, 1])
def test_moments_flat_main_loop_channel_major(extra):
    """Channel-major C = 64 with rows just above the main-loop threshold (extra = 0: rows % 4 == 0, 16-byte loads), and one
    row more (rows % 4 == 1: the planes lose their alignment and every element goes through the scalar loop, many grid
    passes)."""
    from vbq_amd import ops
    C = 64
    gx, need = LP.moments_flat_grid(1_000_000, C)
    rows = 4 * (need + gx * LP.THREADS // 2) + extra
    assert LP.moments_flat_grid(rows, C) == (gx, need) and rows // 4 > need and rows % 4 == extra
    rng = np.random.default_rng(12 + extra)
    x = rng.standard_normal((C, rows), dtype=np.float32) * (1 + np.arange(C, dtype=np.float32))[:, None] + np.float32(0.1)
    got = ops.moments(torch.from_numpy(x).cuda(), layout="cb").cpu().numpy()
    assert got.shape == (C, 2)
    _check_moments(got, x)


def test_moments_channel_last_at_the_declared_channel_limit():
    """Channel-last (33, 4096): n_ch = 4096 is the declared limit (64 KB of dynamic LDS in k_moments_bc); 4097 is refused."""
    from vbq_amd import _lib, ops
    rows, C = 33, LP.MOMENTS_MAX_CH
    gx, stride = LP.moments_bc_grid(rows, C)
    assert gx * LP.THREADS >= C and stride % C == 0 and stride < rows * C          # every lane walks several rows
    rng = np.random.default_rng(14)
    x = rng.standard_normal((rows, C), dtype=np.float32) * np.float32(2) - np.float32(0.5)
    got = ops.moments(torch.from_numpy(x).cuda(), layout="bc").cpu().numpy()
    assert got.shape == (C, 2)
    _check_moments(got, np.ascontiguousarray(x.T))
    with pytest.raises(_lib.VBQError, match="n_ch <= 4096"):
        ops.moments(torch.zeros((2, C + 1), device="cuda"), layout="bc")


@pytest.mark.parametrize("layout", ["bc", "cb"])
def test_rd_sums_grid_stride_accumulation(cus, layout):
    """More elements than the capped grid has lanes (two and a half passes), L = 9 (two chunks of lambdas, the second with
    one), with a per-lambda rate table, a shared one and none.  The terms are non-negative and each is formed with at most 8
    roundings, so any order of summing E of them stays within (E + 8) * 2^-53 of the exact sum, relatively (factor 2 as above)."""
    from vbq_amd import ops
    N, C, L = 10, 16, 9
    T = 2 ** (N + 1) - 1
    cap = LP.rd_sums_grid(1 << 40, L, cus)[0]
    rows = LP.cdiv(cap * LP.THREADS * 5 // 2, C) + 1
    E = rows * C
    gx, chunks, passes = LP.rd_sums_grid(E, L, cus)
    assert gx == cap and chunks == 2 and passes == 3 and E % (gx * LP.THREADS) != 0
    rng = np.random.default_rng(21)
    shape = (rows, C) if layout == "bc" else (C, rows)
    ch = (np.arange(C)[None, :] if layout == "bc" else np.arange(C)[:, None]) + np.zeros(shape, np.int64)
    mu = rng.normal(0, 1.2, shape).astype(np.float32)
    sg = np.exp(rng.normal(-2, 0.7, shape)).astype(np.float32)
    srt = np.sort(rng.normal(0, 1.5, (C, T)).astype(np.float32), axis=1)
    idx = rng.integers(0, T, (L,) + shape).astype(np.uint16)
    idx[L - 1].reshape(-1)[-3:] = [0, T - 1, 65535]                  # the last elements of the last pass; 65535 reads entry T - 1
    rate = np.abs(rng.normal(6, 3, (L, C, T))).astype(np.float32)
    q = np.minimum(idx.astype(np.int64), T - 1)
    ld = np.longdouble
    w = 1 / (2 * sg.astype(ld) ** 2)
    want_d = np.stack([_exact(((srt[ch, q[l]].astype(ld) - mu.astype(ld)) ** 2 * w).reshape(-1).astype(np.float64)) for l in range(L)])
    want_r = np.stack([_exact(rate[l][ch, q[l]].reshape(-1).astype(np.float64)) for l in range(L)])
    want_r0 = np.stack([_exact(rate[0][ch, q[l]].reshape(-1).astype(np.float64)) for l in range(L)])
    rel = 2.0 * (E + 8) * 2.0 ** -53
    d = [torch.from_numpy(a).cuda() for a in (mu, sg, idx, srt, rate)]
    for r, want in ((d[4], want_r), (d[4][0].contiguous(), want_r0), (None, np.zeros(L))):
        got = ops.rd_sums(d[0], d[1], d[2], d[3], C, N=N, layout=layout, rate=r).cpu().numpy()
        assert got.shape == (L, 2)
        assert np.all(np.abs(got[:, 0] - want_d) <= rel * want_d), (got[:, 0], want_d)
        assert np.all(np.abs(got[:, 1] - want) <= rel * want), (got[:, 1], want)


SCAN_N = (1 << 21) + 3


def test_index_max_second_and_third_grid_pass():
    """n = 2^21 + 3: the capped grid of 2^20 lanes passes twice over the array and three lanes a third time.  The maximum is
    planted where only the later passes read it: first and last element of the second pass, last element of all."""
    from vbq_amd import ops
    gx, passes = LP.scan_grid(SCAN_N)
    lanes = gx * LP.THREADS
    assert (gx, passes) == (LP.SCAN_WGS, 3) and lanes == 1 << 20
    g = torch.Generator(device="cuda").manual_seed(31)
    base = torch.randint(0, 1000, (SCAN_N,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    assert ops.index_max(base.view(torch.uint16)) == int(base.max())
    for k, pos in enumerate((lanes, 2 * lanes - 1, 2 * lanes, SCAN_N - 1)):
        x = base.clone()
        value = 60000 + k
        x[pos] = value - 65536                                       # the u16 value as int16 bits
        assert ops.index_max(x.view(torch.uint16)) == value, f"maximum at element {pos} not seen"


def test_check_inputs_second_and_third_grid_pass():
    """The same array length: bad means and spreads only at elements the second and third grid pass read; exact counts."""
    from vbq_amd import ops
    lanes = LP.scan_grid(SCAN_N)[0] * LP.THREADS
    assert LP.scan_grid(SCAN_N) == (LP.SCAN_WGS, 3)
    g = torch.Generator(device="cuda").manual_seed(32)
    mu = torch.randn(SCAN_N, device="cuda", generator=g)
    sg = torch.rand(SCAN_N, device="cuda", generator=g) + 0.01
    ops.check_inputs(mu, sg)                                         # clean: no exception
    inf, nan = float("inf"), float("nan")
    for pos, v in ((lanes, nan), (lanes + 7, inf), (SCAN_N - 1, -inf)):
        mu[pos] = v
    for pos, v in ((lanes + 1, 0.0), (2 * lanes - 1, -1.0), (2 * lanes, inf), (SCAN_N - 2, nan), (SCAN_N - 1, -0.0)):
        sg[pos] = v
    with pytest.raises(ValueError, match=r"invalid latents: 3 non-finite means, 5 standard deviations"):
        ops.check_inputs(mu, sg)
    mu[lanes], mu[lanes + 7], mu[SCAN_N - 1] = 0.0, 1.0, -1.0
    with pytest.raises(ValueError, match=r"invalid latents: 0 non-finite means, 5 standard deviations"):
        ops.check_inputs(mu, sg)


_HIST_SHAPE = (10, 20_000, 40, 32)                                  # N, rows, C, L
_hist_cases = {}


def _hist_case(content):
    """(idx u16 [L, rows, C], np.bincount counts [L, C, T]) -- made once, shared by the two counter widths."""
    if content not in _hist_cases:
        N, rows, C, L = _HIST_SHAPE
        T = 2 ** (N + 1) - 1
        rng = np.random.default_rng(41)
        idx = rng.integers(0, T, (L, rows, C), dtype=np.uint16)
        if content == "one_bin":
            hot = rng.integers(0, T, C, dtype=np.uint16)
            hot[:3] = [0, T - 1, T // 2]
            idx = np.where(rng.random((L, rows, C), dtype=np.float32) < 0.9, hot[None, None, :], idx)
        flat = (np.arange(L, dtype=np.int64)[:, None, None] * C + np.arange(C, dtype=np.int64)[None, None, :]) * T + idx
        want = np.bincount(flat.reshape(-1), minlength=L * C * T).reshape(L, C, T)
        assert int(want.sum()) == L * rows * C
        _hist_cases[content] = (idx, want)
    return _hist_cases[content]


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
@pytest.mark.parametrize("content", ["uniform", "one_bin"])
def test_histogram_channel_last_several_row_passes(content, dtype):
    """Channel-last rows = 20 000, C = 40, L = 32: three channel groups (the last of eight channels), six workgroups per
    group and lambda, each over 53 passes of 64 rows; uniform indices and 90 % of them in one bin per channel (LDS atomics on
    one address), int64 and int32 counters -- against np.bincount."""
    from vbq_amd import ops
    N, rows, C, L = _HIST_SHAPE
    gx, groups, passes = LP.hist_tiled_grid(rows, C, L)
    assert gx >= 2 and groups == 3 and passes >= 3 and rows % (gx * LP.HIST_TILED_ROWS) != 0
    idx, want = _hist_case(content)
    got = ops.histogram(torch.from_numpy(idx).cuda(), C, N=N, layout="bc", dtype=dtype)
    assert got.dtype == dtype and np.array_equal(got.cpu().numpy(), want)
