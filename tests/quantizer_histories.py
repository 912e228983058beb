"""Histories of one ChannelwisePriorCDFQuantizer: states, probes and the fresh oracle.

vbq_amd/quantizer.py keeps device tables, codecs, captured graphs and staging buffers between calls and decides itself when an
event -- a rebuilt model, a new code-point table, a replaced dict entry, a larger batch -- makes one of them stale.  The property
the tests hold it to is exact: WHATEVER A QUANTIZER WAS ASKED BEFORE, ITS ANSWER EQUALS THE ANSWER OF A QUANTIZER BUILT ONCE, IN
THE FINAL STATE, AND ASKED ONLY THIS.  Files and lengths are compared byte for byte, tensors bit for bit.

A STATE is a recipe fixed by seeds (code-point table, fit latents, lambdas, add_n_smoothing, an optional replaced model);
`fresh(state)` builds a new quantizer from it and `move(q, new, old)` takes a living one there through the public API.  C and N
are the same in every state, so every cached tensor keeps its shape and dtype across a transition.
A PROBE is a named function probe(q, inputs) -> tuple of bytes, ints and NumPy arrays; `outcome` runs one and also records the
documented errors (KeyError, ValueError, TypeError, VBQError), `same` compares two outcomes exactly.
INPUTS hold the latents of a few files, class maps, palettes and budgets; the budgets are derived from a fresh quantizer's own
coded_nbytes* answers (a length strictly between two rungs), never constants.

FAILED_ATTEMPTS are the calls that raise -- transitions refused half way, probes asked what they must refuse -- each with the
exception type it raises; tests/test_gpu_failed_calls.py holds the quantizer to answering every probe afterwards as before.
PROBED / EXEMPT say, for every public method of the class, which probes call it or why none does;
tests/test_quantizer_histories_host.py holds them against the class.  A NEW PUBLIC METHOD OF THE QUANTIZER GOES INTO ONE OF THE
TWO.  Importable without a GPU."""
import zipfile
from collections import namedtuple

import numpy as np

C, N = 4, 6
T = 2 ** (N + 1) - 1
SEGMENT, PART = 64, 256                       # every file of FILE_SHAPES but the smallest has several segments; file 0 several parts
SCALES = np.linspace(0.5, 2.0, C)             # of the Gaussian grid, per channel (as tests/test_gpu_api.py builds its table)
FIT_ROWS = 3000
LAMBS_A = (0.01, 0.05, 0.3, 1.5, 7.0, 30.0)
NEW, DROPPED = 0.2, (0.3, 30.0)               # Lsub: a reordered strict subset of LAMBS_A plus NEW; DROPPED are the ones left out
LAMBS_SUB = (7.0, 0.05, NEW, 1.5, 0.01)
REPLACED = 0.3                                # R: the lambda whose two model arrays are replaced
FILE_SHAPES = ((24, 24, C), (7, C), (3, 5, C), (2, 4, 9, C), (130, C))
IMAGE_SHAPES = ((1, 6, 10, 3), (1, 9, 5, 3), (1, 3, 4, 3))          # NHWC images; the stub VAE keeps the leading axes for its latents


# ------------------------------------------------------------------------------------------------------------------ states
State = namedtuple("State", "name clamp fit lambs smoothing replaced")
STATES = {s.name: s for s in (
    State("A", None, "A", LAMBS_A, 1, None),
    State("B", None, "B", LAMBS_A, 1, None),
    State("S2", None, "A", LAMBS_A, 2, None),
    State("Lsub", None, "A", LAMBS_SUB, 1, None),
    State("E", 1.5, "A", LAMBS_A, 1, None),           # the grid clamped to +-1.5 sigma: the outer code points of a channel coincide
    State("E2", 1.0, "A", LAMBS_A, 1, None),          # a second non-strict table (the sensitivity control of canon_u16 needs two)
    State("R", None, "A", LAMBS_A, 1, REPLACED),
)}


class Grid:
    """The prior build_code_points asks: a Gaussian ppf grid with one scale per channel, clamped to +-clamp sigma when given."""

    def __init__(self, clamp=None):
        self.clamp = clamp

    def inverse_cdf(self, xi):
        from scipy.stats import norm
        pts = norm.ppf(np.asarray(xi, np.float64)) * SCALES[None, :]
        if self.clamp is not None:
            pts = np.clip(pts, -self.clamp * SCALES[None, :], self.clamp * SCALES[None, :])
        return pts


def code_points(state):
    """The table of the state as build_code_points stores it: f32 [C, T], level-major."""
    from vbq_amd.tables import n_bit_binary_floats
    xi = np.hstack([n_bit_binary_floats(n) for n in range(N + 1)])
    return np.ascontiguousarray(Grid(state.clamp).inverse_cdf(np.repeat(xi[:, None], C, axis=1)).astype(np.float32).T)


def fit_latents(kind):
    """(means, logvars) f32 [FIT_ROWS, C] the entropy models are fitted on.  A: means of the prior's own spread, narrow
    posteriors; B: means concentrated near 0, wide posteriors -- every lambda's frequency table differs between the two."""
    rng = np.random.default_rng({"A": 101, "B": 202}[kind])
    if kind == "A":
        means, logvars = rng.normal(0, 1, (FIT_ROWS, C)) * SCALES, rng.normal(-4.0, 0.5, (FIT_ROWS, C))
    else:
        means, logvars = rng.normal(0, 0.15, (FIT_ROWS, C)), rng.normal(-0.5, 0.5, (FIT_ROWS, C))
    return means.astype(np.float32), logvars.astype(np.float32)


def replacement(q, lamb):
    """The public edit the docstring of _keyed_dev recommends: NEW arrays under the key of `lamb` in both model dicts."""
    em = np.array(q.entropy_models[lamb], dtype=np.float32) + np.float32(0.5)
    rm = np.array(q.raw_code_length_entropy_models[lamb], dtype=np.float32) + np.linspace(0, 1.5, N + 1, dtype=np.float32)[None, :]
    q.entropy_models[lamb] = em
    q.raw_code_length_entropy_models[lamb] = rm


def move(q, new, old=None):
    """Take q from state `old` (None: just constructed) to state `new` through the public API only: build_code_points when the
    table changes, build_entropy_models_from_latents when anything fitted changes, the dict replacements of R."""
    if old is None or old.clamp != new.clamp:
        q.build_code_points(Grid(new.clamp))
    if old is None or (old.clamp, old.fit, old.lambs, old.smoothing) != (new.clamp, new.fit, new.lambs, new.smoothing) \
            or old.replaced is not None:
        means, logvars = fit_latents(new.fit)
        q.build_entropy_models_from_latents(means, logvars, list(new.lambs), new.smoothing, spread="logvar")
    if new.replaced is not None:
        replacement(q, new.replaced)
    return q


def fresh(state):
    """A new quantizer built only from the recipe."""
    from vbq_amd import ChannelwisePriorCDFQuantizer
    return move(ChannelwisePriorCDFQuantizer(C, N), state)


# ------------------------------------------------------------------------------------------------------------------ inputs
def latents(shapes, seed=7):
    """One (posterior_means, posterior_logvars) pair f32 per shape."""
    rng = np.random.default_rng(seed)
    return [((rng.normal(0, 1.2, sh) * SCALES).astype(np.float32), rng.normal(-4.0, 0.6, sh).astype(np.float32)) for sh in shapes]


def class_maps(shapes, P, seed=11):
    """One class map per shape, integers in [0, P) shaped like the latents without the channel axis; every class of the palette
    occurs where the map has at least P positions."""
    rng = np.random.default_rng(seed + P)
    out = []
    for sh in shapes:
        m = rng.integers(0, P, int(np.prod(sh[:-1])))
        m[:P] = np.arange(P)[:m.size]
        out.append(m.reshape(sh[:-1]).astype(np.int64))
    return out


def interior_budget(lengths, want, strict=True):
    """A budget strictly between two rungs: lengths[j] <= budget < min(lengths[:j]) for a rung j >= 1 -- `want` where the lengths
    allow it, else the nearest rung that does -- so the first rung that fits is j.  Files of a row or two can have one length at
    every rung: strict=False then returns lengths[0] (the first rung fits), strict=True raises."""
    lengths = [int(v) for v in lengths]
    rungs = [j for j in range(1, len(lengths)) if min(lengths[:j]) - lengths[j] >= 2]
    if not rungs:
        if strict:
            raise AssertionError(f"no two rungs of {lengths} leave room for a budget between them")
        return lengths[0]
    j = min(rungs, key=lambda r: (abs(r - want), r))
    return lengths[j] + (min(lengths[:j]) - lengths[j]) // 2


class Inputs:
    """What the probes are asked with.  ls: the lambdas they may name, ascending; every probe names ls[2].
    files: F pairs of latents (NumPy, or device tensors after .on_device()); cls2 / cls3: their class maps for palettes of 2 and 3;
    ladder: candidate palettes of 2 (bitstream.palette_ladder); budgets: see make_inputs; given: files written beforehand, for the
    reader probes ({"b" | "c" | "m": [F files]}; None: a reader writes its own with the quantizer it reads with)."""

    def __init__(self, ls, files, cls2, cls3, budgets, tag):
        from vbq_amd import bitstream
        self.ls = [float(l) for l in ls]
        ls = self.ls
        F = len(files)
        self.files, self.cls2, self.cls3, self.budgets, self.tag = list(files), list(cls2), list(cls3), dict(budgets), tag
        self.lamb = ls[2]
        self.lambs = [ls[2], ls[0], ls[3]]                                   # several rates, not in order
        self.file_lambs = [ls[(2, 0, 2, 3, 1)[f % 5]] for f in range(F)]     # one per file, repeats
        self.palette2, self.palette3 = (ls[2], ls[0]), (ls[1], ls[2], ls[3])
        self.file_palettes = [((ls[2], ls[0]), (ls[0], ls[2]), (ls[1], ls[2]))[f % 3] for f in range(F)]
        self.ladder = bitstream.palette_ladder(ls, (0, 1))
        self.given = None
        self.form = "numpy"
        self.image_form = None

    def _copy(self):
        new = object.__new__(Inputs)
        new.__dict__.update(self.__dict__)
        return new

    def on_device(self):
        """The same inputs with every latent a device tensor."""
        import torch
        new = self._copy()
        new.files = [(torch.from_numpy(m).cuda(), torch.from_numpy(lv).cuda()) for m, lv in self.files]
        new.form, new.tag = "device", self.tag + "/device"
        return new

    def in_form(self, form, which, values_only=False):
        """The same inputs with one group of arrays in a form of tests/input_forms.py: `which` is "files" (the latents), "cls2",
        "cls3", "X" (the image the WITH_VAE probes encode) or "all".  values_only: the PLAIN form (C-contiguous NumPy; device
        tensors when these inputs are on the device) of form.values(a) -- what the answer under the form is held against.
        The budgets, lambdas and palettes stay as they are."""
        import input_forms as IF
        assert which in ("files", "cls2", "cls3", "X", "all"), which
        plain = IF.DEV_PLAIN if self.form == "device" else IF.NP_PLAIN

        def host(a):
            return np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)

        def to(a, base=plain):
            a = host(a)
            if not form.applies(a):
                return base.make(a)
            return base.make(form.values(a)) if values_only else form.make(a)
        new = self._copy()
        if which in ("files", "all"):
            new.files = [(to(m), to(lv)) for m, lv in self.files]
        for name in ("cls2", "cls3"):
            if which in (name, "all"):
                setattr(new, name, [to(c, IF.NP_PLAIN) for c in getattr(self, name)])
        if which in ("X", "all") and form.family != "device":
            new.image_form = (lambda a: IF.NP_PLAIN.make(form.values(a))) if values_only else \
                (lambda a: form.make(a) if form.applies(a) else a)
        new.tag = f"{self.tag}/{form.name}:{which}" + ("/values" if values_only else "")
        return new

    def image(self, X):
        """The image a WITH_VAE probe encodes, in the form in_form(form, "X") asked for."""
        return X if self.image_form is None else self.image_form(np.asarray(X))

    def reading(self, given, tag):
        """The same inputs for the reader probes, with the files they read given."""
        new = self._copy()
        new.given, new.tag = given, self.tag + "/" + tag
        return new


def make_inputs(oracle, ls, shapes=FILE_SHAPES, tag="files", strict=True):
    """Inputs for the files of `shapes` whose budgets come from `oracle`'s own exact lengths: for every family a length strictly
    between two rungs, the rung interior and differing from file to file where the lengths allow it.
    budgets: one / one_c / one_m: file 0 alone in segments, compact, lambda-map; batch / compact / mapped: one per file;
    total / compact_total / mapped_total: all files together."""
    ls = sorted(float(l) for l in ls)
    files, cls2, cls3 = latents(shapes), class_maps(shapes, 2), class_maps(shapes, 3)
    inp = Inputs(ls, files, cls2, cls3, {}, tag)
    F, L, K = len(files), len(ls), len(inp.ladder)
    if F == 0:
        inp.budgets = dict(one=1, one_c=1, one_m=1, batch=[], compact=[], mapped=[], total=1, compact_total=1, mapped_total=1)
        return inp
    nb = np.array([[d[l] for l in ls] for d in oracle.coded_nbytes_batch(files, ls, segment=SEGMENT)], np.int64)
    nc = np.array([[d[l] for l in ls] for d in oracle.coded_nbytes_compact_batch(files, ls, part=PART)], np.int64)
    nm = np.asarray(oracle.coded_nbytes_mapped_palettes_batch(files, inp.ladder, cls2, segment=SEGMENT), np.int64)
    assert nb.shape == nc.shape == (F, L) and nm.shape == (F, K)
    want = lambda f, n: 1 + f % max(1, n - 2)                                  # interior rungs, another one from file to file
    inp.budgets = dict(
        # (file 0 alone and the totals take the rung of ls[2] -- in the ladder the candidate (ls[1], ls[2]) -- so that these
        # probes name ls[2] as all others do)
        one=interior_budget(nb[0], 2, strict), one_c=interior_budget(nc[0], 2, strict), one_m=interior_budget(nm[0], 1, strict),
        batch=[interior_budget(nb[f], want(f, L), strict) for f in range(F)],
        compact=[interior_budget(nc[f], want(f + 1, L), strict) for f in range(F)],
        mapped=[interior_budget(nm[f], want(f, K), strict) for f in range(F)],
        total=interior_budget(nb.sum(axis=0), 2, strict), compact_total=interior_budget(nc.sum(axis=0), 2, strict),
        mapped_total=interior_budget(nm.sum(axis=0), 1, strict))
    return inp


class StubVAE:
    """The tiny VAE of the replay test in tests/test_gpu_api.py: torch code on the device whose latents depend on the image (so a
    captured graph that replays stale inputs shows); the latents keep the image's leading axes."""

    def __init__(self, image_shape, seed=5):
        import torch
        rng = np.random.default_rng(seed + int(np.prod(image_shape)))
        sh = tuple(image_shape[:-1]) + (C,)
        self.means = torch.from_numpy((rng.normal(0, 1.2, sh) * SCALES).astype(np.float32)).cuda()
        self.logvars = torch.from_numpy(rng.normal(-4.0, 0.6, sh).astype(np.float32)).cuda()

    def encode(self, X):
        import torch
        # (an image in any form -- a strided or reversed array, a list, a CPU tensor -- as one dense f32 device tensor, so that
        # the mean is the same reduction whatever the form)
        X = X.detach() if isinstance(X, torch.Tensor) else torch.from_numpy(np.array(X, np.float32, order="C"))
        X = X.to("cuda", torch.float32).contiguous()
        return self.means + X.mean(), self.logvars

    def decode(self, Z):
        return (0.1 * Z.mean(dim=-1, keepdim=True) + 0.5).repeat_interleave(3, dim=-1)


def image(shape, seed=3):
    return np.random.default_rng(seed + int(np.prod(shape))).uniform(0, 1, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ outcomes
def _plain(v):
    """A probe's result as nested tuples of bytes, ints, floats, strings and NumPy arrays."""
    if isinstance(v, (bytes, str, int, float, np.integer, np.floating)) or v is None:
        return v
    if isinstance(v, (bytearray, memoryview)):
        return bytes(v)
    if isinstance(v, dict):
        return tuple((_plain(k), _plain(x)) for k, x in v.items())
    if isinstance(v, (list, tuple)):
        return tuple(_plain(x) for x in v)
    if hasattr(v, "detach") and hasattr(v, "cpu"):                          # a torch tensor
        v = v.detach().cpu()
        import torch
        if v.dtype in (torch.uint16, torch.uint32, torch.uint64):
            return v.view({torch.uint16: torch.int16, torch.uint32: torch.int32, torch.uint64: torch.int64}[v.dtype]).numpy().copy()
        return v.numpy().copy()
    return np.array(v)                                                       # ndarrays and the lazy views of vbq_amd.lazy


def outcome(probe, q, inp):
    """("ok", the result) or ("raised", the error's type name, its message) for the errors the methods document."""
    from vbq_amd._lib import VBQError
    try:
        return ("ok", _plain(probe(q, inp)))
    except (KeyError, ValueError, TypeError, VBQError) as e:
        return ("raised", type(e).__name__, str(e))


def same(a, b):
    """Exact equality of two outcomes: bytes and ints by value, arrays by dtype, shape and every bit."""
    if isinstance(a, tuple) or isinstance(b, tuple):
        return isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and a.tobytes() == b.tobytes())
    return type(a) is type(b) and a == b


# ------------------------------------------------------------------------------------------------------------------ probes
def _one(i):
    return i.files[0]


def _flat(i):
    """File 0 as rows [B, C] of means and standard deviations, NumPy."""
    m, lv = (np.asarray(a.detach().cpu() if hasattr(a, "cpu") else a) for a in _one(i))
    return m.reshape(-1, C), np.exp(0.5 * lv.reshape(-1, C).astype(np.float64)).astype(np.float32)


def _lead(a):
    """`a` with a leading axis of one (a nested list gets it as a list)."""
    return [a] if isinstance(a, list) else a[None]


def p_latents(q, i):
    m, lv = _one(i)
    out = q.compress_latents(_lead(m), _lead(lv), i.lambs)
    return tuple(np.asarray(out[k][l]) for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits") for l in out[k])


def p_latents_mapped(q, i):
    m, lv = _one(i)
    out = q.compress_latents_mapped(m, lv, i.palette3, i.cls3[0])
    return out["Z_hat"], out["num_bits"]


def p_batch_channel(q, i):
    mu, sd = _flat(i)
    zs, bs = q.compress_batch_channel_latents(mu, sd, i.lambs)
    return tuple(np.asarray(zs[l]) for l in i.lambs) + tuple(np.asarray(bs[l]) for l in i.lambs)


def p_intervals(q, i):
    return q.get_all_N_bit_intervals(_flat(i)[0])


def p_codec(q, i):
    mu, sd = _flat(i)
    words, sizes, cdc = q.encode_batch(mu, sd, i.lambs, segment=SEGMENT)
    back = q.decode_batch(words, sizes, cdc, mu.shape[0], i.lambs)
    return words, sizes, tuple(back[l] for l in i.lambs), q.codec(i.lambs, SEGMENT).freq_host


def _layout_probes(layout, budget):
    def p_to_bytes(q, i):
        m, lv = _one(i)
        return (q.compress_latents_to_bytes(m, lv, i.lamb, segment=SEGMENT, layout=layout, part=PART),)

    def p_coded_nbytes(q, i):
        m, lv = _one(i)
        return q.coded_nbytes(m, lv, i.ls, segment=SEGMENT, layout=layout, part=PART), \
            q.coded_nbytes(m, lv, [i.lamb], segment=SEGMENT, layout=layout, part=PART)

    def p_to_budget(q, i):
        m, lv = _one(i)
        return (q.compress_latents_to_budget(m, lv, i.budgets[budget], i.ls, segment=SEGMENT, layout=layout, part=PART),)
    return p_to_bytes, p_coded_nbytes, p_to_budget


p_to_bytes, p_coded_nbytes, p_to_budget = _layout_probes("segments", "one")
p_to_bytes_c, p_coded_nbytes_c, p_to_budget_c = _layout_probes("interleaved", "one_c")


def p_to_bytes_mapped(q, i):
    m, lv = _one(i)
    return (q.compress_latents_to_bytes_mapped(m, lv, i.palette2, i.cls2[0], segment=SEGMENT),
            q.compress_latents_to_bytes_mapped(m, lv, i.palette3, i.cls3[0], segment=SEGMENT))


def p_coded_nbytes_mapped(q, i):
    m, lv = _one(i)
    return (q.coded_nbytes_mapped(m, lv, i.palette2, i.cls2[0], segment=SEGMENT),
            q.coded_nbytes_mapped(m, lv, i.palette3, i.cls3[0], segment=SEGMENT))


def p_nbytes_palettes(q, i):
    m, lv = _one(i)
    return (q.coded_nbytes_mapped_palettes(m, lv, i.ladder, i.cls2[0], segment=SEGMENT),)


def p_to_budget_mapped(q, i):
    m, lv = _one(i)
    return (q.compress_latents_to_budget_mapped(m, lv, i.budgets["one_m"], i.ladder, i.cls2[0], segment=SEGMENT),)


# ---- batches, written
def b_to_bytes(q, i):
    return (q.compress_latents_to_bytes_batch(i.files, i.file_lambs, segment=SEGMENT),)


def b_coded_nbytes(q, i):
    return (q.coded_nbytes_batch(i.files, i.ls, segment=SEGMENT),)


def b_to_budget(q, i):
    return (q.compress_latents_to_budget_batch(i.files, i.budgets["batch"], i.ls, segment=SEGMENT),)


def b_total_budget(q, i):
    return q.compress_latents_to_total_budget(i.files, i.budgets["total"], i.ls, segment=SEGMENT)


def b_compact(q, i):
    return (q.compress_latents_to_compact_batch(i.files, i.file_lambs, part=PART),)


def b_coded_nbytes_compact(q, i):
    return (q.coded_nbytes_compact_batch(i.files, i.ls, part=PART),)


def b_compact_budget(q, i):
    return (q.compress_latents_to_compact_budget_batch(i.files, i.budgets["compact"], i.ls, part=PART),)


def b_compact_total_budget(q, i):
    return q.compress_latents_to_compact_total_budget(i.files, i.budgets["compact_total"], i.ls, part=PART)


def b_mapped(q, i):
    return (q.compress_latents_to_bytes_mapped_batch(i.files, i.file_palettes, i.cls2, segment=SEGMENT),
            q.compress_latents_to_bytes_mapped_batch(i.files, i.palette3, i.cls3, segment=SEGMENT))


def b_coded_nbytes_mapped(q, i):
    return (q.coded_nbytes_mapped_batch(i.files, i.file_palettes, i.cls2, segment=SEGMENT),)


def b_nbytes_palettes(q, i):
    return (q.coded_nbytes_mapped_palettes_batch(i.files, i.ladder, i.cls2, segment=SEGMENT),)


def b_mapped_budget(q, i):
    return (q.compress_latents_to_budget_mapped_batch(i.files, i.budgets["mapped"], i.ladder, i.cls2, segment=SEGMENT),)


def b_mapped_total_budget(q, i):
    return q.compress_latents_to_total_budget_mapped(i.files, i.budgets["mapped_total"], i.ladder, i.cls2, segment=SEGMENT)


# ---- readers.  The files they read: i.given, or written here by the one-file calls of the quantizer that reads them.
WINDOWS = (((slice(3, 17), slice(5, 20)), None), ((slice(8, 11), slice(0, 4)), [3, 1]), ((slice(None), slice(None)), None))
"""(region, channels) of the window readers on file 0 (24 x 24): a box, a smaller box with a channel subset, the whole file."""


def written(q, i, kind, f):
    """File f of i.files in one format: "b" (segments), "c" (compact) or "m" (lambda map, a palette of two)."""
    if i.given is not None:
        return i.given[kind][f]
    m, lv = i.files[f]
    if kind == "m":
        return q.compress_latents_to_bytes_mapped(m, lv, i.file_palettes[f], i.cls2[f], segment=SEGMENT)
    return q.compress_latents_to_bytes(m, lv, i.file_lambs[f], segment=SEGMENT, layout="segments" if kind == "b" else "interleaved",
                                       part=PART)


def written_all(q, i):
    """Every file of i.files in every format: {"b" | "c" | "m": [F files]}."""
    return {kind: [written(q, i, kind, f) for f in range(len(i.files))] for kind in "bcm"}


# Regions of the batch readers.  The extents of one call must agree, so a call takes files with as many leading axes: files 0 and
# 2 (two axes), then files 1 and 4 (one axis; the box of file 4 crosses a segment boundary).
BOXES_2D = [(slice(10, 13), slice(2, 6)), (slice(0, 3), slice(1, 5))]
BOXES_1D = [(slice(1, 7),), (slice(60, 66),), (slice(100, 106),)]


def r_decompress_b(q, i):
    return tuple(q.decompress_latents(written(q, i, "b", f)) for f in (0, 3))


def r_decompress_c(q, i):
    return tuple(q.decompress_latents(written(q, i, "c", f)) for f in (0, 3))


def r_decompress_m(q, i):
    return tuple(q.decompress_latents(written(q, i, "m", f)) for f in (0, 3))


def r_window(q, i):
    data = written(q, i, "b", 0)
    return tuple(q.decompress_latents_window(data, region, channels) for region, channels in WINDOWS)


def r_batch(q, i):
    b = {f: written(q, i, "b", f) for f in (0, 2, 1, 4)}
    return (q.decompress_latents_batch([b[0], b[2]], regions=BOXES_2D),
            q.decompress_latents_batch([b[1], b[4], b[4]], regions=BOXES_1D, channels=[2, 0, 2]),
            q.decompress_latents_batch([b[0], b[0]]))


def r_mapped_window(q, i):
    data = written(q, i, "m", 0)
    return tuple(q.decompress_latents_mapped_window(data, region, channels) for region, channels in WINDOWS)


def r_mapped_batch(q, i):
    m = {f: written(q, i, "m", f) for f in (0, 2, 1, 4)}
    return (q.decompress_latents_mapped_batch([m[0], m[2]], regions=BOXES_2D),
            q.decompress_latents_mapped_batch([m[1], written(q, i, "b", 4), m[4]], regions=BOXES_1D, channels=[1, 3]),
            q.decompress_latents_mapped_batch([m[0], m[0]]))


def r_compact_batch(q, i):
    return (q.decompress_latents_compact_batch([written(q, i, "c", f) for f in range(len(i.files))], stack=False),)


BATCH_READERS = ("r_batch", "r_mapped_batch", "r_compact_batch")
"""The readers whose digest error names the index of the file: every one passes file 0 of the inputs first."""


# ---- with a VAE
_VAES = {}


def _image_probe(shape):
    """The image of a shape and ITS VAE: one object per shape for the whole session, as an evaluation loop keeps one -- the
    replays a quantizer holds are keyed on the VAE's identity, so only a VAE that returns can meet a stale capture."""
    if shape not in _VAES:
        _VAES[shape] = StubVAE(shape)
    return image(shape), _VAES[shape]


def v_replay(q, i, shape=IMAGE_SHAPES[0]):
    X, vae = _image_probe(shape)
    outs = []
    for x in (X, 0.5 * X):                                        # the capture, then a replay of it with another image
        out, (sums, sums_cl, u8) = q.compress_replay(i.image(x), vae, i.lambs)
        outs.append((tuple(np.array(out[k][l]) for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits", "X_hat") for l in out[k]),
                     sums, sums_cl, u8))
    return tuple(outs)


def v_compress(q, i, shape=IMAGE_SHAPES[0]):
    X, vae = _image_probe(shape)
    out = q.compress(i.image(X), vae, i.lambs)
    return tuple(np.asarray(out[k][l]) for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits", "X_hat") for l in out[k])


def v_bytes(q, i, shape=IMAGE_SHAPES[0]):
    X, vae = _image_probe(shape)
    data = q.compress_to_bytes(i.image(X), vae, i.lamb, segment=SEGMENT)
    return data, q.decompress(data, vae)


ONE_LATENT = dict(latents=p_latents, latents_mapped=p_latents_mapped, batch_channel=p_batch_channel, intervals=p_intervals,
                  codec=p_codec)
ONE_FILE = dict(to_bytes=p_to_bytes, coded_nbytes=p_coded_nbytes, to_budget=p_to_budget, to_bytes_c=p_to_bytes_c,
                coded_nbytes_c=p_coded_nbytes_c, to_budget_c=p_to_budget_c, to_bytes_mapped=p_to_bytes_mapped,
                coded_nbytes_mapped=p_coded_nbytes_mapped, nbytes_palettes=p_nbytes_palettes, to_budget_mapped=p_to_budget_mapped)
BATCHES = dict(b_to_bytes=b_to_bytes, b_coded_nbytes=b_coded_nbytes, b_to_budget=b_to_budget, b_total_budget=b_total_budget,
               b_compact=b_compact, b_coded_nbytes_compact=b_coded_nbytes_compact, b_compact_budget=b_compact_budget,
               b_compact_total_budget=b_compact_total_budget, b_mapped=b_mapped, b_coded_nbytes_mapped=b_coded_nbytes_mapped,
               b_nbytes_palettes=b_nbytes_palettes, b_mapped_budget=b_mapped_budget, b_mapped_total_budget=b_mapped_total_budget)
READERS = dict(r_decompress_b=r_decompress_b, r_decompress_c=r_decompress_c, r_decompress_m=r_decompress_m, r_window=r_window,
               r_batch=r_batch, r_mapped_window=r_mapped_window, r_mapped_batch=r_mapped_batch, r_compact_batch=r_compact_batch)
WITH_VAE = dict(v_replay=v_replay, v_compress=v_compress, v_bytes=v_bytes)
PROBES = {**ONE_LATENT, **ONE_FILE, **BATCHES, **READERS, **WITH_VAE}
"""Probe name -> probe.  The probes of ONE_FILE and BATCHES run in both input forms (Inputs.on_device)."""


def runs(inp):
    """Every (name, probe, inputs) of one pass over all probes: each once, the file probes -- one file and batches -- also with
    device tensors."""
    dev = inp.on_device()
    return [(name, p, inp) for name, p in PROBES.items()] + [(name + "[device]", p, dev) for name, p in {**ONE_FILE, **BATCHES}.items()]


# ------------------------------------------------------------------------------------------------------------------ coverage
NO_STATE, WRAPPER, TRANSITION = "reads no state", "pure wrapper of ", "changes the state: the transitions call it"
EXEMPT_REASONS = (NO_STATE, WRAPPER, TRANSITION)
"""The closed set of reasons.  WRAPPER is followed by the name of the probed method it calls after vae.encode."""

PROBED = {
    "get_all_N_bit_intervals": ["intervals"],
    "compress_latents": ["latents"], "compress_latents_mapped": ["latents_mapped"],
    "compress_batch_channel_latents": ["batch_channel"],
    "codec": ["codec"], "encode_batch": ["codec"], "decode_batch": ["codec"],
    "compress_latents_to_bytes": ["to_bytes", "to_bytes_c"], "coded_nbytes": ["coded_nbytes", "coded_nbytes_c"],
    "compress_latents_to_budget": ["to_budget", "to_budget_c"],
    "compress_latents_to_bytes_mapped": ["to_bytes_mapped"], "coded_nbytes_mapped": ["coded_nbytes_mapped"],
    "coded_nbytes_mapped_palettes": ["nbytes_palettes"], "compress_latents_to_budget_mapped": ["to_budget_mapped"],
    "compress_latents_to_bytes_batch": ["b_to_bytes"], "coded_nbytes_batch": ["b_coded_nbytes"],
    "compress_latents_to_budget_batch": ["b_to_budget"], "compress_latents_to_total_budget": ["b_total_budget"],
    "compress_latents_to_compact_batch": ["b_compact"], "coded_nbytes_compact_batch": ["b_coded_nbytes_compact"],
    "compress_latents_to_compact_budget_batch": ["b_compact_budget"],
    "compress_latents_to_compact_total_budget": ["b_compact_total_budget"],
    "compress_latents_to_bytes_mapped_batch": ["b_mapped"], "coded_nbytes_mapped_batch": ["b_coded_nbytes_mapped"],
    "coded_nbytes_mapped_palettes_batch": ["b_nbytes_palettes"],
    "compress_latents_to_budget_mapped_batch": ["b_mapped_budget"],
    "compress_latents_to_total_budget_mapped": ["b_mapped_total_budget"],
    "decompress_latents": ["r_decompress_b", "r_decompress_c", "r_decompress_m"],
    "decompress_latents_window": ["r_window"], "decompress_latents_batch": ["r_batch"],
    "decompress_latents_mapped_window": ["r_mapped_window"], "decompress_latents_mapped_batch": ["r_mapped_batch"],
    "decompress_latents_compact_batch": ["r_compact_batch"],
    "compress_replay": ["v_replay"], "compress": ["v_compress"], "compress_to_bytes": ["v_bytes"], "decompress": ["v_bytes"],
}
"""Public method -> the probes that call it."""

EXEMPT = {
    "build_code_points": TRANSITION, "build_entropy_models_from_latents": TRANSITION, "save": TRANSITION, "load": TRANSITION,
    "build_entropy_models": WRAPPER + "build_entropy_models_from_latents",
    "compress_to_bytes_batch": WRAPPER + "compress_latents_to_bytes_batch",
    "compress_to_compact_batch": WRAPPER + "compress_latents_to_compact_batch",
    "compress_to_bytes_mapped": WRAPPER + "compress_latents_to_bytes_mapped",
    "compress_to_bytes_mapped_batch": WRAPPER + "compress_latents_to_bytes_mapped_batch",
    "compress_to_budget_mapped": WRAPPER + "compress_latents_to_budget_mapped",
    "compress_to_budget_mapped_batch": WRAPPER + "compress_latents_to_budget_mapped_batch",
    "compress_to_budget": WRAPPER + "compress_latents_to_budget",
    "compress_to_budget_batch": WRAPPER + "compress_latents_to_budget_batch",
    "compress_to_compact_budget_batch": WRAPPER + "compress_latents_to_compact_budget_batch",
}
"""Public method -> why no probe calls it (one of EXEMPT_REASONS)."""


def public_methods(cls):
    """The public callables of the class (properties are not callable)."""
    return sorted(name for name in dir(cls) if not name.startswith("_") and callable(getattr(cls, name)))


# ------------------------------------------------------------------------------------------------------------------ failed attempts
FAILED_ATTEMPTS = {}
"""'<public method>:<what is wrong>' -> (function(q, inputs), the exception type the call raises).  The function makes ONE public
call that raises; what it needs before -- a file to damage, a saved state -- it gets from public calls that succeed.  It
restores what it set on the quantizer itself (validate_inputs) and nothing else.  A type given as a string names a class of
vbq_amd._lib (the module imports without the native library); expected_type resolves it."""
UNBUILT = 0.123                                # a lambda no state has a model for
OTHER_STATE = {"A": "E", "E": "A"}             # the state whose files `inputs.foreign` holds in a test of the key
MIDDLE = 2                                     # of the five files of FILE_SHAPES
NEW_IMAGE_SHAPE = (1, 5, 7, 3)                 # not in IMAGE_SHAPES: compress_replay has to capture it


def _attempt(name, exc):
    def register(fn):
        assert name not in FAILED_ATTEMPTS, name
        FAILED_ATTEMPTS[name] = (fn, exc)
        return fn
    return register


def expected_type(exc):
    if isinstance(exc, str):
        from vbq_amd import _lib
        return getattr(_lib, exc)
    return exc


def _with(i, **changes):
    new = i._copy()
    new.__dict__.update(changes)
    return new


def _host(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


# ---- transitions that fail
@_attempt("build_entropy_models_from_latents:lambda_zero", "VBQError")
def t_lambda_zero(q, i):
    # 0.0 is outside the range pass 1's kernels serve: vbq_level_counts_f32 refuses it
    q.build_entropy_models_from_latents(*fit_latents("B"), [0.3, 0.0], 1, spread="logvar")


@_attempt("build_entropy_models_from_latents:33_lambdas_the_last_1e25", "VBQError")
def t_late_lambda(q, i):
    # the offending lambda is in the second chunk of 32; the first chunk is eligible on its own
    q.build_entropy_models_from_latents(*fit_latents("B"), [float(v) for v in np.geomspace(0.01, 30.0, 32)] + [1e25], 1,
                                        spread="logvar")


@_attempt("build_entropy_models_from_latents:one_channel_too_many", ValueError)
def t_channels(q, i):
    means, logvars = (np.pad(a, ((0, 0), (0, 1))) for a in fit_latents("B"))
    q.build_entropy_models_from_latents(means, logvars, list(LAMBS_A), 1, spread="logvar")


@_attempt("build_entropy_models_from_latents:nan_mean_with_validate_inputs", ValueError)
def t_nan_mean(q, i):
    means, logvars = fit_latents("B")
    means = means.copy()
    means[1234, 2] = np.nan
    before, q.validate_inputs = q.validate_inputs, True
    try:
        q.build_entropy_models_from_latents(means, logvars, list(LAMBS_A), 1, spread="logvar")
    finally:
        q.validate_inputs = before


class BadPrior(Grid):
    """Grid(1.25) -- a table of no state -- made wrong in one way: "order" (the two points either side of the median of level 3
    trade places in channel 1: not monotone in xi, before and after the float32 cast), "shape" (a row short), "raises"."""

    def __init__(self, how):
        Grid.__init__(self, 1.25)
        self.how = how

    def inverse_cdf(self, xi):
        if self.how == "raises":
            raise ArithmeticError("this prior has no inverse CDF")
        pts = Grid.inverse_cdf(self, xi)
        if self.how == "shape":
            return pts[:-1]
        lo = 2 ** 3 - 1 + 3
        pts[[lo, lo + 1], 1] = pts[[lo + 1, lo], 1]
        return pts


@_attempt("build_code_points:not_monotone_after_the_f32_cast", ValueError)
def t_not_monotone(q, i):
    q.build_code_points(BadPrior("order"))


@_attempt("build_code_points:wrong_shape", ValueError)
def t_wrong_shape(q, i):
    q.build_code_points(BadPrior("shape"))


@_attempt("build_code_points:inverse_cdf_raises", ArithmeticError)
def t_prior_raises(q, i):
    q.build_code_points(BadPrior("raises"))


def _state_file(q):
    import os
    import tempfile
    path = os.path.join(tempfile.mkdtemp(prefix="vbq_failed_"), "quantizer.npz")
    q.save(path)
    return path


@_attempt("load:truncated_file", zipfile.BadZipFile)
def t_load_truncated(q, i):
    path = _state_file(q)
    with open(path, "rb") as f:
        data = f.read()
    with open(path, "wb") as f:
        f.write(data[:len(data) // 2])              # the archive's directory, which stands at its end, is gone
    type(q).load(path)


@_attempt("load:unknown_format", ValueError)
def t_load_unknown(q, i):
    path = _state_file(q)
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["format"] = np.array("vbq_amd.quantizer/99")
    np.savez_compressed(path, **d)
    type(q).load(path)


@_attempt("save:missing_directory", FileNotFoundError)
def t_save_nowhere(q, i):
    import os
    import tempfile
    q.save(os.path.join(tempfile.mkdtemp(prefix="vbq_failed_"), "no", "such", "directory", "quantizer.npz"))


# ---- probes that raise
@_attempt("compress_latents:unbuilt_lambda", KeyError)
def f_unbuilt(q, i):
    m, lv = _one(i)
    q.compress_latents(m[None], lv[None], [i.lamb, UNBUILT])


@_attempt("compress_replay:unbuilt_lambda_on_a_new_image_shape", KeyError)
def f_replay_abandoned(q, i):
    v_replay(q, _with(i, lambs=[i.lamb, UNBUILT]), NEW_IMAGE_SHAPE)


def _no_rung(probe, key, at=None):
    """The probe with a budget of one byte, which no rung fits (in a batch: for the file in the middle alone)."""
    def fn(q, i):
        b = 1
        if at is not None:
            b = list(i.budgets[key])
            b[at] = 1
        probe(q, _with(i, budgets={**i.budgets, key: b}))
    return fn


for _name, _probe, _key, _at in (
        ("compress_latents_to_budget:no_rung_fits_segments", p_to_budget, "one", None),
        ("compress_latents_to_budget:no_rung_fits_interleaved", p_to_budget_c, "one_c", None),
        ("compress_latents_to_budget_mapped:no_rung_fits", p_to_budget_mapped, "one_m", None),
        ("compress_latents_to_budget_batch:no_rung_fits_the_middle_file", b_to_budget, "batch", MIDDLE),
        ("compress_latents_to_total_budget:no_rung_fits", b_total_budget, "total", None),
        ("compress_latents_to_compact_budget_batch:no_rung_fits_the_middle_file", b_compact_budget, "compact", MIDDLE),
        ("compress_latents_to_compact_total_budget:no_rung_fits", b_compact_total_budget, "compact_total", None),
        ("compress_latents_to_budget_mapped_batch:no_rung_fits_the_middle_file", b_mapped_budget, "mapped", MIDDLE),
        ("compress_latents_to_total_budget_mapped:no_rung_fits", b_mapped_total_budget, "mapped_total", None)):
    _attempt(_name, ValueError)(_no_rung(_probe, _key, _at))


def _bad_file_in_the_middle(probe):
    """A batch writer whose file in the middle has C + 1 channels."""
    def fn(q, i):
        files = list(i.files)
        files[MIDDLE] = tuple(np.concatenate([_host(a), _host(a)[..., :1]], axis=-1) for a in files[MIDDLE])
        probe(q, _with(i, files=files))
    return fn


for _name, _probe in BATCHES.items():
    (_method,) = [m for m, ps in PROBED.items() if _name in ps]
    _attempt(_method + ":bad_file_in_the_middle", ValueError)(_bad_file_in_the_middle(_probe))

# The file each reader is given in place of a good one: (kind, index) -- for the one-file readers the SECOND file they read, for
# the batch readers a file that stands in the middle of a list (r_batch reads [b1, b4, b4], r_mapped_batch [m1, b4, m4],
# r_compact_batch all five).
BAD_FILE_OF = {"r_decompress_b": ("b", 3), "r_decompress_c": ("c", 3), "r_decompress_m": ("m", 3), "r_window": ("b", 0),
               "r_mapped_window": ("m", 0), "r_batch": ("b", 4), "r_mapped_batch": ("b", 4), "r_compact_batch": ("c", MIDDLE)}


def _reader_given(reader, name, bad):
    """The reader on files this quantizer wrote itself, one of them replaced by bad(that file, inputs, kind, index)."""
    def fn(q, i):
        given = written_all(q, i)
        kind, f = BAD_FILE_OF[name]
        given[kind][f] = bad(given[kind][f], i, kind, f)
        reader(q, i.reading(given, "bad"))
    return fn


def _truncated(data, i, kind, f):
    return bytes(data[:len(data) // 2])


def _foreign(data, i, kind, f):
    assert i.foreign is not None, "the test sets inputs.foreign to the files of OTHER_STATE"
    assert i.foreign[kind][f] != data
    return i.foreign[kind][f]


for _name, _reader in READERS.items():
    (_method,) = [m for m, ps in PROBED.items() if _name in ps]
    _kind = BAD_FILE_OF[_name][0]
    _attempt(f"{_method}:damaged_file_{_name}", ValueError)(_reader_given(_reader, _name, _truncated))
    _attempt(f"{_method}:file_of_another_state_{_name}", ValueError)(_reader_given(_reader, _name, _foreign))


@_attempt("decompress_latents_window:region_of_three_axes_in_a_file_of_two", ValueError)
def f_window_axes(q, i):
    # (a slice past the end of an axis is clamped as NumPy clamps it and selects nothing: only a region with an axis the file
    # does not have lies outside it in a way the reader refuses)
    q.decompress_latents_window(written(q, i, "b", 0), (slice(3, 17), slice(5, 20), slice(0, 2)), None)


@_attempt("decompress_latents_mapped_window:channel_outside_the_file", ValueError)
def f_window_channel(q, i):
    q.decompress_latents_mapped_window(written(q, i, "m", 0), (slice(3, 17), slice(5, 20)), [1, C])
