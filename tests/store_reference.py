"""NumPy restatement of vbqs_plan_boxes (vbq_amd/store/vbq_store.h, "Planned boxes") and of the bound the store sizes its segment
lists by.  The lists are built the way the header states it -- run by run, max(lo_r, hi_{r-1} + 1) .. hi_r -- and NOT through
bitstream.box_segments, which tests/test_store_host.py holds them against.  Importable without a GPU and without the library."""
import numpy as np

CUT, BAD_SAMPLE = 32, 128
INT64_MAX, INT32_MAX = (1 << 63) - 1, (1 << 31) - 1


def max_listed_segments(dims, extents, seg):
    (D0, D1, D2), (w0, w1, w2) = (int(d) for d in dims), (int(w) for w in extents)
    if min(w0, w1, w2) <= 0:
        return 0
    nseg = -(-D0 * D1 * D2 // seg)
    return min(nseg, w0 * w1 * ((w2 + seg - 2) // seg + 1), w0 * (((w1 - 1) * D2 + w2 + seg - 2) // seg + 1))


def valid(row, n_files, file_id, origin, extents, seg):
    """The header's validity rule in Python integers -> D0, or None for an invalid sample.  `row`: the table row of the id (any
    row when the id is out of range)."""
    if not 0 <= file_id < n_files:
        return None
    n, D1, D2 = int(row[1]), int(row[2]), int(row[3])
    if n < 0 or D1 < 1 or D2 < 1 or D1 * D2 > INT64_MAX or n % (D1 * D2) or -(-n // seg) > INT32_MAX:
        return None
    D0 = n // (D1 * D2)
    if any(not 0 <= a <= D - w for a, D, w in zip(origin, (D0, D1, D2), extents)):
        return None
    return D0


def box_list(dims, origin, extents, seg):
    """The segments of a valid box, run by run, as a Python list."""
    (D0, D1, D2), (a0, a1, a2), (w0, w1, w2) = dims, origin, extents
    out, hi_prev = [], -1
    for i0 in range(a0, a0 + w0):
        for i1 in range(a1, a1 + w1):
            first = (i0 * D1 + i1) * D2 + a2
            lo, hi = first // seg, (first + w2 - 1) // seg
            out.extend(range(max(lo, hi_prev + 1), hi + 1))
            hi_prev = hi
    return out


def plan_boxes(table, ids, origins, extents, seg, n_sel):
    """-> (desc int64 [S, fields], segs int32 [S, n_sel], status u32 [S]) as vbqs_plan_boxes writes them into zeroed status
    words.  With an empty box or n_sel == 0 the call launches nothing: None."""
    table = np.asarray(table, np.int64)
    ids, origins = [int(v) for v in np.asarray(ids).reshape(-1)], np.asarray(origins, np.int64).reshape(-1, 3)
    extents = tuple(int(w) for w in extents)
    S, (F, fields) = len(ids), table.shape
    if min(extents) == 0 or n_sel == 0:
        return None
    desc, segs, status = np.zeros((S, fields), np.int64), np.full((S, n_sel), -1, np.int32), np.zeros(S, np.uint32)
    for s, f in enumerate(ids):
        origin = tuple(int(a) for a in origins[s])
        row = table[f] if 0 <= f < F else table[0]
        D0 = valid(row, F, f, origin, extents, seg)
        if D0 is None:
            desc[s] = table[0]
            desc[s, 4:7] = 0
            status[s] = BAD_SAMPLE
            continue
        desc[s] = row
        desc[s, 4:7] = origin
        lst = box_list((D0, int(row[2]), int(row[3])), origin, extents, seg)
        if len(lst) > n_sel:
            status[s] |= CUT
        segs[s, :min(len(lst), n_sel)] = lst[:n_sel]
    return desc, segs, status


def synthetic_table(dims_list, fields, seg, rng, C=3):
    """A table of `fields` fields for files of the geometries dims_list: seg_base as C streams per file would give it, the
    fields after the geometry filled with small distinct values, so that a row copied from the wrong place shows."""
    t = np.zeros((len(dims_list), fields), np.int64)
    base = 0
    for f, (D0, D1, D2) in enumerate(dims_list):
        n = D0 * D1 * D2
        t[f, :4] = (base, n, D1, D2)
        t[f, 7:] = rng.integers(1, 1000, fields - 7)
        base += C * -(-n // seg)
    return t


def random_samples(dims_list, extents, S, rng):
    """S valid samples: ids over the files that hold the extents, origins uniform over each file's valid range, corners
    included."""
    ok = [f for f, d in enumerate(dims_list) if all(w <= D for w, D in zip(extents, d))]
    assert ok
    ids = rng.choice(ok, S)
    origins = np.array([[int(rng.integers(0, D - w + 1)) for D, w in zip(dims_list[f], extents)] for f in ids], np.int64)
    return ids.astype(np.int64), origins.reshape(S, 3)
