"""The resident latent store on the GPU: vbqs_plan_boxes against its NumPy restatement (tests/store_reference.py) between
canary guards, and LatentStore against decompress_latents -- every sample of a crop bit for bit the slice of the full decode.
Everything here is exact: integer equality or bit patterns, no tolerance.

vbq_amd/store lies outside the scans of tests/dirty_memory.py, tests/footprint.py and tests/stream_order.py (they enumerate
include/vbq.h, vbq_amd/csrc and the top-level modules); the cases below carry those guarantees for it: the canary guards, the
two dirty fills, the late-input harness and the synchronisation check."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as DM  # noqa: E402
import footprint as FP  # noqa: E402
import store_reference as SR  # noqa: E402
import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu
N, C32, SEG = 10, 32, 64
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
SHAPES = [(1, 16, 48, C32), (2, 9, 23, C32), (1, 20, 30, C32), (1, 12, 40, C32), (1, 3, 150, C32), (37, C32), (2, 2, 5, 7, C32)]
DIMS = [(1, 16, 48), (2, 9, 23), (1, 20, 30), (1, 12, 40), (1, 3, 150), (1, 1, 37), (4, 5, 7)]
PALETTES = [[LAMBS[3], LAMBS[0]], [LAMBS[2]], [LAMBS[1], LAMBS[3], LAMBS[0], LAMBS[2]], [LAMBS[2], LAMBS[0], LAMBS[3]],
            [LAMBS[1]], [LAMBS[0], LAMBS[2]], [LAMBS[3]]]
KINDS = [b"VBQm", b"VBQb", b"VBQm", b"VBQm", b"VBQb", b"VBQm", b"VBQb"]
PLAIN = [(1, LAMBS[0]), (2, LAMBS[3]), (4, LAMBS[2]), (5, LAMBS[1]), (0, LAMBS[3])]     # (latent, lambda) of the b"VBQb" store
CHANNELS = [None, [C32 - 1, 0, 5, 5]]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _quantizer(seed, smoothing=1):
    """The recipe of tests/test_gpu_mapped_window.py::world: a factored Gaussian prior, models built from latent 0."""
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C32))
    q = ChannelwisePriorCDFQuantizer(C32, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C32), scale))
    lat = [((scale * rng.standard_normal(s)).astype(np.float32), (2 * (-2 + 0.7 * rng.standard_normal(s))).astype(np.float32))
           for s in SHAPES]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, C32), lat[0][1].reshape(-1, C32), LAMBS, add_n_smoothing=smoothing,
                                        spread="logvar")
    return q, lat, rng


class World:
    """One quantizer, seven latents, their files at segment 64 (mixed) and a second set of b"VBQb" files at other lambdas, the
    full decode of each reshaped to (D0, D1, D2, C), and a store over each set: shared, never changed."""

    def __init__(self):
        from vbq_amd.store import LatentStore
        self.q, self.lat, rng = _quantizer(7)
        q = self.q
        self.classes = [rng.integers(0, len(p), s[:-1]) for p, s in zip(PALETTES, SHAPES)]
        self.files = [q.compress_latents_to_bytes(m, lv, pal[0], segment=SEG) if kind == b"VBQb" else
                      q.compress_latents_to_bytes_mapped(m, lv, pal, cl, segment=SEG)
                      for (m, lv), pal, cl, kind in zip(self.lat, PALETTES, self.classes, KINDS)]
        assert [bytes(d[:4]) for d in self.files] == KINDS
        self.full = [q.decompress_latents(d).reshape(dims + (C32,)) for d, dims in zip(self.files, DIMS)]
        self.store = LatentStore(q, self.files)
        self.plain_files = [q.compress_latents_to_bytes(*self.lat[i], lam, segment=SEG) for i, lam in PLAIN]
        self.plain_dims = [DIMS[i] for i, _ in PLAIN]
        self.plain_full = [q.decompress_latents(d).reshape(dims + (C32,)) for d, dims in zip(self.plain_files, self.plain_dims)]
        self.plain_store = LatentStore(q, self.plain_files)

    def pick(self, which):
        return ((self.store, self.full, DIMS) if which == "mixed" else (self.plain_store, self.plain_full, self.plain_dims))


@pytest.fixture(scope="module")
def world():
    return World()


def want_crops(full, ids, origins, box, channels=None):
    ch = slice(None) if channels is None else list(channels)
    return np.stack([full[f][a0:a0 + box[0], a1:a1 + box[1], a2:a2 + box[2]][..., ch]
                     for f, (a0, a1, a2) in zip(ids.tolist(), origins.tolist())])


def corner_samples(dims_list, box, rng, extra=24):
    """Every corner (0 and D - w per level) of every file that holds the box, then seeded origins; shuffled, with repeats."""
    ids, origins = [], []
    for f, d in enumerate(dims_list):
        if all(w <= D for w, D in zip(box, d)):
            for corner in sorted({tuple(k * (D - w) for k, D, w in zip(ks, d, box)) for ks in np.ndindex(2, 2, 2)}):
                ids.append(f), origins.append(corner)
    more = SR.random_samples(dims_list, box, extra, rng)
    ids, origins = np.concatenate([np.array(ids, np.int64), more[0]]), np.concatenate([np.array(origins, np.int64).reshape(-1, 3), more[1]])
    order = rng.permutation(ids.size)
    return ids[order], origins[order]


# ====================================================================================================== the kernel alone
K_DIMS = [(12, 17, 40), (2, 3, 5), (11, 15, 37), (10, 14, 150)]
RUNS = [(1, 1), (7, 9), (8, 8), (5, 13), (10, 14)]                       # w0 w1 = 1, 63, 64, 65, 140: the carry between chunks


def _plan(table, ids, origins, box, seg, n_sel, off):
    """One vbqs_plan_boxes between guards -> (desc, segs, status as NumPy); the guards are checked."""
    from vbq_amd import store
    S, fields = len(ids), table.shape[1]
    g = [FP.Guarded((S, fields), torch.int64, "cuda", off), FP.Guarded((S, n_sel), torch.int32, "cuda", off),
         FP.Guarded((S,), torch.uint32, "cuda", off).fill(np.zeros(S, np.uint32))]
    store.plan_boxes(torch.from_numpy(table).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(origins).cuda(), box, seg=seg,
                     n_sel=n_sel, desc=g[0].view, segs=g[1].view, status=g[2].view)
    torch.cuda.synchronize()
    for x, what in zip(g, ("desc", "segs", "status")):
        x.assert_outside_intact(f"{what} box={box} seg={seg} n_sel={n_sel} offset={off}")
    return g[0].host(), g[1].host(), g[2].host()


@pytest.mark.parametrize("fields", [8, 16])
@pytest.mark.parametrize("seg", [1, 7, 64])
def test_plan_equals_the_restatement(seg, fields):
    """Seeded ids and origins over files of four geometries: descriptors, lists and status word for word, at 1, 63, 64, 65 and
    140 runs, runs of 1, seg + 1 and more than 2 seg rows, n_sel at the bound and 3 above it; outputs aligned and one element
    off, between guards."""
    rng = np.random.default_rng([seg, fields])
    table = SR.synthetic_table(K_DIMS, fields, seg, rng)
    case = 0
    for (w0, w1) in RUNS:
        for w2 in (1, seg + 1, 2 * seg + 2):
            box = (w0, w1, w2)
            ids, origins = SR.random_samples(K_DIMS, box, 37, rng)
            bound = max(SR.max_listed_segments(d, box, seg) for d in K_DIMS)
            for n_sel in (bound, bound + 3):
                want = SR.plan_boxes(table, ids, origins, box, seg, n_sel)
                got = _plan(table, ids, origins, box, seg, n_sel, case & 1)
                for w, g, what in zip(want, got, ("desc", "segs", "status")):
                    assert np.array_equal(w, g), (what, box, seg, n_sel, np.argwhere(w != g)[:4])
                assert not want[2].any() and (want[1][:, -1] == -1).all() == (n_sel > max((r >= 0).sum() for r in want[1]))
                case += 1


@pytest.mark.parametrize("fields", [8, 16])
def test_invalid_samples_are_flagged_alone_and_read_row_zero(fields):
    rng = np.random.default_rng(fields)
    seg, box = 7, (2, 3, 9)
    table = SR.synthetic_table(K_DIMS, fields, seg, rng)
    table[1] = table[0]
    table[1, 1] += 1                                                      # row 1: n % (D1 D2) != 0
    F = len(K_DIMS)
    good = lambda f: [int(rng.integers(0, D - w + 1)) for D, w in zip(K_DIMS[f], box)]
    edge = [D - w for D, w in zip(K_DIMS[2], box)]
    samples = [(0, good(0)), (-1, good(0)), (3, good(3)), (F, good(0)), (1 << 40, good(0)), (2, good(2)), (0, [0, -1, 0]),
               (2, edge), (2, [edge[0] + 1, edge[1], edge[2]]), (2, [edge[0], edge[1] + 1, edge[2]]), (2, [edge[0], edge[1], edge[2] + 1]),
               (3, [1 << 62, 0, 0]), (3, [0, 0, 1 << 62]), (0, [1 << 62] * 3), (1, [0, 0, 0]), (3, good(3)), (-(1 << 62), good(0))]
    bad = [1, 3, 4, 6, 8, 9, 10, 11, 12, 13, 14, 16]
    ids, origins = np.array([s[0] for s in samples], np.int64), np.array([s[1] for s in samples], np.int64)
    n_sel = max(SR.max_listed_segments(d, box, seg) for d in K_DIMS) + 1
    want = SR.plan_boxes(table, ids, origins, box, seg, n_sel)
    assert np.flatnonzero(want[2]).tolist() == bad and set(want[2][bad].tolist()) == {128}
    desc, segs, status = _plan(table, ids, origins, box, seg, n_sel, 1)
    assert np.array_equal(status, want[2]) and np.array_equal(segs, want[1]) and np.array_equal(desc, want[0])
    assert (segs[bad] == -1).all() and (desc[bad] == np.concatenate([table[0, :4], [0, 0, 0], table[0, 7:]])).all()
    for s in sorted(set(range(len(samples))) - set(bad)):                 # the neighbours, stated without the restatement
        assert desc[s].tolist() == table[ids[s], :4].tolist() + origins[s].tolist() + table[ids[s], 7:].tolist()
        assert segs[s][segs[s] >= 0].tolist() == SR.box_list(K_DIMS[ids[s]], tuple(origins[s].tolist()), box, seg)


def test_a_list_one_longer_than_n_sel_is_cut_and_flagged():
    rng = np.random.default_rng(11)
    seg, box = 7, (3, 5, 9)
    table = SR.synthetic_table(K_DIMS, 8, seg, rng)
    ids, origins = SR.random_samples(K_DIMS, box, 9, rng)
    need = [len(SR.box_list(K_DIMS[f], tuple(o), box, seg)) for f, o in zip(ids.tolist(), origins.tolist())]
    n_sel = max(need) - 1
    want = SR.plan_boxes(table, ids, origins, box, seg, n_sel)
    assert [int(s) for s in want[2]] == [32 if n > n_sel else 0 for n in need] and 32 in want[2] and (want[1][np.array(need) > n_sel] >= 0).all()
    for off in (0, 1):
        got = _plan(table, ids, origins, box, seg, n_sel, off)            # (the guard after the last row is checked there)
        assert all(np.array_equal(w, g) for w, g in zip(want, got))
    one = _plan(table, ids[:1], origins[:1], box, seg, 1, 1)              # a row of one entry
    assert one[1].tolist() == [[SR.box_list(K_DIMS[ids[0]], tuple(origins[0]), box, seg)[0]]] and one[2].tolist() == [32]


def test_refused_arguments_return_the_code_and_write_nothing():
    from vbq_amd import _lib_store, ops
    rng = np.random.default_rng(5)
    table = torch.from_numpy(SR.synthetic_table(K_DIMS, 8, 7, rng)).cuda()
    ids, origins = (torch.from_numpy(a).cuda() for a in SR.random_samples(K_DIMS, (1, 2, 3), 5, rng))
    g = [FP.Guarded((5, 8), torch.int64, "cuda"), FP.Guarded((5, 4), torch.int32, "cuda"), FP.Guarded((5,), torch.uint32, "cuda")]
    base = dict(table=ops._ptr(table), n_files=4, fields=8, ids=ops._ptr(ids), origins=ops._ptr(origins), S=5, w0=1, w1=2, w2=3,
                seg=7, n_sel=4, desc=g[0].ptr, segs=g[1].ptr, status=g[2].ptr)
    for bad in (dict(fields=7), dict(fields=12), dict(n_files=0), dict(S=-1), dict(w1=-1), dict(seg=0), dict(seg=65534),
                dict(n_sel=-1), dict(table=None), dict(ids=None), dict(origins=None), dict(status=None)):
        a = {**base, **bad}
        rc = _lib_store.lib().vbqs_plan_boxes(*[a[k] for k in ("table", "n_files", "fields", "ids", "origins", "S", "w0", "w1", "w2",
                                                               "seg", "n_sel", "desc", "segs", "status")], ops._stream(table))
        assert rc == -1 and b"vbqs_plan_boxes" in _lib_store.lib().vbqs_last_error(), bad
    torch.cuda.synchronize()
    for x in g:
        x.assert_untouched("a refused call")


# ====================================================================================================== the store
@pytest.mark.parametrize("channels", CHANNELS, ids=["all", "listed"])
@pytest.mark.parametrize("box", [(1, 8, 8), (1, 1, 1), (2, 9, 23), (1, 3, 130)])
@pytest.mark.parametrize("which", ["mixed", "plain"])
def test_crops_are_the_slices_of_the_full_decode(world, which, box, channels):
    store, full, dims = world.pick(which)
    rng = np.random.default_rng([len(dims), *box])
    ids, origins = corner_samples(dims, box, rng)
    if box == (2, 9, 23):
        assert set(ids.tolist()) == {dims.index((2, 9, 23))}              # only that file holds it: a whole file
    want = want_crops(full, ids, origins, box, channels)
    out, status = store.crops(torch.from_numpy(ids).cuda(), torch.from_numpy(origins).cuda(), box, channels=channels)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == want.shape
    assert status.dtype == torch.uint32 and not status.cpu().numpy().any()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    store.check(status, ids)
    got = store.read(ids.tolist(), origins.tolist(), box, channels=channels, return_np=True)      # host lists
    assert isinstance(got, np.ndarray) and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("which", ["mixed", "plain"])
def test_the_short_form_and_the_empty_results(world, which):
    store, full, dims = world.pick(which)
    rng = np.random.default_rng(31)
    ids, origins = corner_samples(dims, (1, 8, 8), rng)
    origins[:, 0] = 0
    want = want_crops(full, ids, origins, (1, 8, 8), CHANNELS[1])[:, 0]
    out, status = store.crops(torch.from_numpy(ids).cuda(), torch.from_numpy(origins[:, 1:].copy()).cuda(), (8, 8), channels=CHANNELS[1])
    assert tuple(out.shape) == (ids.size, 8, 8, 4) and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    given = torch.full((ids.size, 8, 8, 4), 3.0, device="cuda")
    st = torch.zeros(ids.size, dtype=torch.uint32, device="cuda")
    out2, st2 = store.crops(ids, origins[:, 1:], (8, 8), channels=CHANNELS[1], out=given, status=st)
    assert out2 is given and st2 is st and np.array_equal(_bits(given.cpu().numpy()), _bits(want))
    for args, shape in (((ids[:0], origins[:0], (1, 8, 8)), (0, 1, 8, 8, C32)), ((ids, origins, (1, 0, 8)), (ids.size, 1, 0, 8, C32)),
                        ((ids, origins[:, 1:], (8, 0)), (ids.size, 8, 0, C32))):
        out, status = store.crops(*args)
        assert tuple(out.shape) == shape and tuple(status.shape) == (len(args[0]),) and not status.cpu().numpy().any()
    out, _ = store.crops(ids, origins, (1, 8, 8), channels=[])
    assert tuple(out.shape) == (ids.size, 1, 8, 8, 0)
    assert (store.n_files, store.segment, store.shapes) == (len(dims), SEG, [tuple(s) for s in (SHAPES if which == "mixed" else
                                                                                                 [SHAPES[i] for i, _ in PLAIN])])
    assert store.nbytes > sum(len(d) for d in (world.files if which == "mixed" else world.plain_files)) // 2 and store.device.type == "cuda"
    with pytest.raises(ValueError, match="channels must be integers"):
        store.crops(ids, origins, (1, 8, 8), channels=[C32])


def test_an_invalid_sample_keeps_the_given_out_and_check_names_it(world):
    store, full, dims = world.pick("mixed")
    rng = np.random.default_rng(41)
    ids, origins = SR.random_samples(dims, (1, 8, 8), 6, rng)
    ids[2], origins[4, 2] = len(dims), dims[ids[4]][2] - 8 + 1             # a file that is not there; a box one column out
    fill = torch.full((6, 1, 8, 8, C32), 7.5, device="cuda")
    out, status = store.crops(torch.from_numpy(ids).cuda(), torch.from_numpy(origins).cuda(), (1, 8, 8), out=fill)
    st, got = status.cpu().numpy(), out.cpu().numpy()
    assert [int(v) & 128 for v in st] == [0, 0, 128, 0, 128, 0] and not st[[0, 1, 3, 5]].any()
    assert (got[[2, 4]] == 7.5).all()
    keep = [0, 1, 3, 5]
    assert np.array_equal(_bits(got[keep]), _bits(want_crops(full, ids[keep], origins[keep], (1, 8, 8))))
    with pytest.raises(ValueError, match=r"sample 2 \(file 7\)"):
        store.check(status, torch.from_numpy(ids).cuda())
    with pytest.raises(ValueError, match=r"sample 2\b"):
        store.check(status)
    with pytest.raises(ValueError, match=r"sample 2 \(file 7\)"):
        store.read(ids, origins, (1, 8, 8))


def _flip_final_state(data, c, g):
    """`data` (a lambda-map file) with the high half of the final state of segment g of channel c flipped in one bit (as
    tests/test_gpu_mapped_window.py plants it)."""
    from vbq_amd import bitstream
    h, _, sizes, start = bitstream.parse_mapped(data)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    e = c * h.nseg + g
    flipped = bytearray(data)
    flipped[start + 2 * (int(offs[e]) + int(sizes[e]) - 1) + 1] ^= 0x40
    return bytes(flipped)


def test_damage_inside_a_crop_is_flagged_on_the_samples_that_touch_it_and_outside_only_verify_sees_it(world):
    from vbq_amd import _lib
    from vbq_amd.store import LatentStore
    q, files, full = world.q, world.files, world.full
    box = (1, 8, 8)
    # file 2: 20 x 30 in segments of 64; segment 2 holds positions 128..191, segment 8 positions 512..575 (rows 17..19)
    ids = np.array([0, 2, 2, 1, 2, 3, 2], np.int64)
    origins = np.array([[0, 3, 11], [0, 3, 11], [0, 8, 0], [1, 1, 9], [0, 0, 20], [0, 4, 30], [0, 6, 5]], np.int64)
    lists = [SR.box_list(DIMS[f], tuple(o), box, SEG) for f, o in zip(ids.tolist(), origins.tolist())]
    touch = [f == 2 and 2 in l for f, l in zip(ids.tolist(), lists)]
    assert touch == [False, True, False, False, True, False, True] and not any(f == 2 and 8 in l for f, l in zip(ids.tolist(), lists))
    want = want_crops(full, ids, origins, box)
    inside = LatentStore(q, files[:2] + [_flip_final_state(files[2], 3, 2)] + files[3:])
    out, status = inside.crops(ids, origins, box)
    st = status.cpu().numpy()
    assert [bool(v) for v in st] == touch
    clean = [i for i, t in enumerate(touch) if not t]
    assert np.array_equal(_bits(out.cpu().numpy()[clean]), _bits(want[clean]))
    with pytest.raises(_lib.VBQError, match=r"sample 1 \(file 2\): rANS bitstream rejected"):
        inside.check(status, ids)
    with pytest.raises(_lib.VBQError, match=r"sample \d+ \(file 2\)"):
        inside.read(torch.from_numpy(ids).cuda(), torch.from_numpy(origins).cuda(), box)
    # the channels the damage does not touch still decode
    got, st = inside.crops(ids, origins, box, channels=[2, 4])
    assert not st.cpu().numpy().any() and np.array_equal(_bits(got.cpu().numpy()), _bits(want[..., [2, 4]]))
    outside = LatentStore(q, files[:2] + [_flip_final_state(files[2], 3, 8)] + files[3:])
    got, st = outside.crops(ids, origins, box)
    assert not st.cpu().numpy().any() and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    with pytest.raises(_lib.VBQError, match=r"sample \d+ \(file 2\)"):
        outside.verify()
    world.store.verify()
    world.plain_store.verify()


def test_more_samples_than_one_launch_takes(world, monkeypatch):
    """65 537 boxes of one position, one channel: two plan launches and two decode launches into one out and one status."""
    from vbq_amd import ops, store as store_mod
    store, full, dims = world.pick("plain")
    S = 65537
    rng = np.random.default_rng(65537)
    ids, origins = SR.random_samples(dims, (1, 1, 1), S, rng)
    counts = {"plan": [], "decode": []}
    real_plan, real_decode = store_mod.plan_boxes, ops.rans_decode_window

    def plan(table, i, *a, **k):
        counts["plan"].append(i.shape[0])
        return real_plan(table, i, *a, **k)

    def decode(*a, **k):
        counts["decode"].append(a[3].shape[0])
        return real_decode(*a, **k)
    monkeypatch.setattr(store_mod, "plan_boxes", plan)
    monkeypatch.setattr(ops, "rans_decode_window", decode)
    out, status = store.crops(torch.from_numpy(ids).cuda(), torch.from_numpy(origins).cuda(), (1, 1, 1), channels=[0])
    assert counts == {"plan": [65535, 2], "decode": [65535, 2]}
    assert tuple(out.shape) == (S, 1, 1, 1, 1) and not status.cpu().numpy().any()
    want = np.empty(S, np.float32)
    for f in range(len(dims)):
        m = ids == f
        want[m] = full[f][origins[m, 0], origins[m, 1], origins[m, 2], 0]
    assert np.array_equal(_bits(out.cpu().numpy().reshape(-1)), _bits(want))


def test_files_the_store_refuses(world):
    from vbq_amd.store import LatentStore
    q, files, lat = world.q, world.files, world.lat
    compact = q.compress_latents_to_bytes(*lat[1], LAMBS[2], layout="interleaved")
    assert bytes(compact[:4]) == b"VBQc"
    with pytest.raises(ValueError, match=r"file 1 is a compact file"):
        LatentStore(q, [files[0], compact])
    with pytest.raises(ValueError, match=r"file 2 is in segments of 32 symbols, file 0 in segments of 64"):
        LatentStore(q, [files[0], files[1], q.compress_latents_to_bytes(*lat[1], LAMBS[2], segment=32)])
    other, other_lat, _ = _quantizer(8)
    foreign = other.compress_latents_to_bytes(*other_lat[1], LAMBS[2], segment=SEG)
    with pytest.raises(ValueError, match=r"file 1 was compressed with a different quantizer or entropy model"):
        LatentStore(q, [files[1], foreign])
    with pytest.raises(ValueError, match="at least one file"):
        LatentStore(q, [])


def test_a_store_outlives_a_rebuild_of_its_quantizers_models():
    from vbq_amd.store import LatentStore
    q, lat, rng = _quantizer(9)
    files = [q.compress_latents_to_bytes(*lat[1], LAMBS[1], segment=SEG),
             q.compress_latents_to_bytes_mapped(*lat[3], PALETTES[3], rng.integers(0, 3, SHAPES[3][:-1]), segment=SEG)]
    store = LatentStore(q, files)
    ids, origins = np.array([1, 0, 1], np.int64), np.array([[0, 2, 7], [1, 0, 3], [0, 4, 32]], np.int64)
    before = store.read(ids, origins, (1, 8, 8), return_np=True)
    full = [q.decompress_latents(d).reshape(dims + (C32,)) for d, dims in zip(files, (DIMS[1], DIMS[3]))]
    assert np.array_equal(_bits(before), _bits(want_crops(full, ids, origins, (1, 8, 8))))
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, C32), lat[0][1].reshape(-1, C32), LAMBS, add_n_smoothing=3, spread="logvar")
    assert np.array_equal(_bits(store.read(ids, origins, (1, 8, 8), return_np=True)), _bits(before))
    store.verify()
    with pytest.raises(ValueError, match=r"file 0 was compressed with a different quantizer or entropy model \(digest mismatch\)"):
        LatentStore(q, files)


def test_sample_draws_valid_boxes_deterministically(world):
    store, full, dims = world.pick("mixed")
    gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
    for box in ((1, 8, 8), (2, 4, 6), (1, 3, 130), (1, 1, 1)):
        ids, origins = store.sample(4000, box, generator=gen(3))
        again = store.sample(4000, box, generator=gen(3))
        assert ids.is_cuda and ids.dtype == torch.int64 and origins.dtype == torch.int64 and tuple(origins.shape) == (4000, 3)
        assert torch.equal(ids, again[0]) and torch.equal(origins, again[1])
        other = store.sample(4000, box, generator=gen(4))
        assert not (torch.equal(ids, other[0]) and torch.equal(origins, other[1]))
        i, o = ids.cpu().numpy(), origins.cpu().numpy()
        holds = [f for f, d in enumerate(dims) if all(w <= D for w, D in zip(box, d))]
        assert set(i.tolist()) == set(holds)                              # every file that can, none that cannot
        room = np.array([[D - w for D, w in zip(dims[f], box)] for f in i])
        assert (o >= 0).all() and (o <= room).all()
        for f in holds if box in ((1, 8, 8), (2, 4, 6)) else ():          # both ends of every level's range are drawn: at most 41
            of = o[i == f]                                                # values per level, about a thousand draws per file
            assert (of.min(axis=0) == 0).all() and (of.max(axis=0) == [D - w for D, w in zip(dims[f], box)]).all()
        _, st = store.crops(ids[:64], origins[:64], box)
        assert not st.cpu().numpy().any()
    ids, origins = store.sample(500, (8, 8), generator=gen(5))
    assert tuple(origins.shape) == (500, 2)
    _, st = store.crops(ids, origins, (8, 8))
    assert not st.cpu().numpy().any() and 1 in ids.cpu().tolist()
    with pytest.raises(ValueError, match="no resident file can hold"):
        store.sample(4, (1, 21, 8))
    assert tuple(store.sample(0, (1, 8, 8))[1].shape) == (0, 3)


@pytest.mark.parametrize("byte", [0x3C, 0xC3])
def test_answers_do_not_depend_on_what_fresh_memory_held(world, byte):
    """Construction, crops, read, sample and verify under dirty_memory.Fill answer bit for bit as they do unpatched."""
    from vbq_amd.store import LatentStore

    def run():
        store = LatentStore(world.q, world.files)
        gen = torch.Generator(device="cuda").manual_seed(12)
        ids, origins = store.sample(40, (1, 8, 8), generator=gen)
        out, status = store.crops(ids, origins, (1, 8, 8), channels=CHANNELS[1])
        whole = store.read([1, 1], [[0, 0, 0]] * 2, (2, 9, 23), return_np=True)
        short = store.read(ids, origins[:, 1:].contiguous(), (8, 8))
        store.verify()
        return tuple(_bits(t.cpu().numpy()) if t.dtype == torch.float32 else t.cpu().numpy()
                     for t in (ids, origins, out, status, short)) + (_bits(whole),)
    clean = run()
    with DM.Fill(byte):
        dirty = run()
    assert len(clean) == len(dirty) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
                                            for a, b in zip(clean, dirty))
    assert np.array_equal(clean[5][0], _bits(world.full[1]))


# ====================================================================================================== stream order, no synchronisation
@pytest.fixture(scope="module")
def spin():
    sp, notes = SO.calibrate()
    print(f"\n[test_gpu_store] {sp}: {notes}")
    return sp


@pytest.mark.parametrize("which", ["mixed", "plain"])
def test_crops_with_device_ids_is_ordered_on_the_callers_stream(world, spin, which):
    """Ids and origins arrive LATE on a side stream (tests/stream_order.py): the call must return while the delay is still
    running, and both of its launches must wait for it."""
    store, full, dims = world.pick(which)
    make = lambda seed: tuple(torch.from_numpy(a).cuda() for a in SR.random_samples(dims, (1, 8, 8), 48, np.random.default_rng(seed)))
    late = SO.run_late(lambda inp: store.crops(inp[0], inp[1], (1, 8, 8)), make(7), make(SO.STALE_SEED), blocking=False, spin=spin,
                       name=f"store.crops[{which}]")
    assert late.armed
    ids, origins = (t.cpu().numpy() for t in make(7))
    assert np.array_equal(late.got[0], _bits(want_crops(full, ids, origins, (1, 8, 8)))) and not late.got[1].any()


def test_crops_with_device_ids_does_not_synchronise(world):
    store, full, dims = world.pick("mixed")
    ids, origins = (torch.from_numpy(a).cuda() for a in SR.random_samples(dims, (1, 8, 8), 32, np.random.default_rng(2)))
    store.crops(ids, origins, (1, 8, 8), channels=CHANNELS[1])            # the channel list is uploaded the first time it is seen
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            enforced = False
        except RuntimeError:
            enforced = True
        if enforced:
            out, status = store.crops(ids, origins, (1, 8, 8))
            out2, _ = store.crops(ids, origins[:, 1:], (8, 8), channels=CHANNELS[1])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not enforced:
        pytest.skip("this torch build does not enforce set_sync_debug_mode('error'): .item() did not raise under it")
    store.check(status, ids)
    want = want_crops(full, ids.cpu().numpy(), origins.cpu().numpy(), (1, 8, 8))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
