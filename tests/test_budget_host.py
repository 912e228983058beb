"""Rate control on the host: the exact file lengths of bitstream.latent_nbytes / embeddings_nbytes against len(write(...)) /
len(write_embeddings(...)), the byte-budget rule and its max_bytes checks, and the argument checks of vbq_rans_sizes_u16 and of
the other five entry points over (n_streams, n, N, seg) (callable without a device)."""
import math

import numpy as np
import pytest

from vbq_amd import bitstream as bs

T10 = 2 ** 11 - 1


def _latent_file(shape, C, segment, rng):
    nseg = (math.prod(shape) // C + segment - 1) // segment
    sizes = rng.integers(2, segment + 3, C * nseg)
    n_words = int(sizes.sum())
    h = bs.Header(N=10, C=C, shape=tuple(shape), lamb=0.5, segment=segment, digest=bytes(range(16)), n_words=n_words)
    return bs.write(h, sizes, rng.integers(0, 2 ** 16, n_words).astype(np.uint16)), n_words


@pytest.mark.parametrize("shape,C,segment", [((7,), 7, 1), ((5, 3), 3, 1), ((1000, 2), 2, 7), ((4, 9), 9, 2),
                                             ((2, 17, 23, 32), 32, 1024), ((1, 32, 48, 256), 256, 37),
                                             ((3, 5, 7, 11), 11, 65533), ((2, 3, 1, 5), 5, 65533)])
def test_latent_nbytes_is_the_written_length(shape, C, segment):
    rng = np.random.default_rng(len(shape) * 1000 + segment + C)
    data, n_words = _latent_file(shape, C, segment, rng)
    assert bs.latent_nbytes(shape, C, segment, n_words) == len(data)
    h, sizes, off = bs.parse(data)
    assert h.n_words == n_words and off + 2 * n_words == len(data)


def _table(K, rng):
    cuts = np.sort(rng.choice(np.arange(1, bs.PROB_ONE), K - 1, replace=False))
    t = np.empty(K, dtype=bs.TABLE_DTYPE)
    t["rank"] = np.sort(rng.choice(T10, K, replace=False))
    t["freq"] = np.diff(np.concatenate([[0], cuts, [bs.PROB_ONE]]))
    t["value"] = np.sort(rng.normal(size=K)).astype(np.float32)
    return t


@pytest.mark.parametrize("shape,segment", [((1000,), 1), ((37,), 65533), ((777, 13), 1000), ((50, 3, 7), 64),
                                           ((2, 3, 4, 5), 1), ((100_000, 3), 65533)])
@pytest.mark.parametrize("K", [2, 3, 100, T10])
def test_embeddings_nbytes_is_the_written_length(shape, segment, K):
    rng = np.random.default_rng(segment + K + len(shape))
    nseg = (math.prod(shape) + segment - 1) // segment
    sizes = rng.integers(2, segment + 3, nseg)
    n_words = int(sizes.sum())
    h = bs.EmbeddingHeader(N=10, shape=shape, segment=segment, beta=1.5, empirical_std=0.7, n_words=n_words, K=K)
    data = bs.write_embeddings(h, _table(K, rng), sizes, rng.integers(0, 2 ** 16, n_words).astype(np.uint16))
    assert bs.embeddings_nbytes(shape, segment, K, n_words) == len(data)
    assert bs.parse_embeddings(data)[0].n_words == n_words


def test_nbytes_reject_what_the_writers_reject():
    with pytest.raises(ValueError, match="channel-last"):
        bs.latent_nbytes((4, 5), 4, 16, 10)
    with pytest.raises(ValueError, match="segment"):
        bs.latent_nbytes((4, 5), 5, 0, 10)
    with pytest.raises(ValueError, match="K = 1"):
        bs.embeddings_nbytes((10, 3), 30, 1, 4)
    with pytest.raises(ValueError, match="empty"):
        bs.embeddings_nbytes((10, 0), 30, 2, 4)


def test_budget_rule_takes_the_smallest_rate_that_fits():
    sizes = {0.25: 1200, 0.5: 900, 1.0: 700, 2.0: 750, 4.0: 600}          # not monotone between 1 and 2
    assert bs.smallest_rate_within(sizes, 10 ** 9) == 0.25
    assert bs.smallest_rate_within(sizes, 1200) == 0.25
    assert bs.smallest_rate_within(sizes, 1199) == 0.5
    assert bs.smallest_rate_within(sizes, 899) == 1.0
    assert bs.smallest_rate_within(sizes, 749) == 1.0                      # 2.0 does not fit, the smaller 1.0 does
    assert bs.smallest_rate_within(sizes, 699) == 4.0
    assert bs.smallest_rate_within(sizes, np.int64(600)) == 4.0
    with pytest.raises(ValueError, match=r"599 bytes: the smallest file is 600 bytes, at lambda = 4\.0"):
        bs.smallest_rate_within(sizes, 599)
    with pytest.raises(ValueError, match=r"at beta = 1\.0"):             # a tie for the smallest file: the smaller rate
        bs.smallest_rate_within({4.0: 600, 1.0: 600}, 10, "beta")
    keys = [np.float32(0.5), np.float32(2.0)]                              # the caller's key objects come back
    assert bs.smallest_rate_within(dict(zip(keys, [5, 3])), 4) is keys[1]
    with pytest.raises(ValueError, match="no candidate"):
        bs.smallest_rate_within({}, 10)


@pytest.mark.parametrize("bad,err", [(True, TypeError), (False, TypeError), (np.bool_(True), TypeError), (10.0, TypeError),
                                     (np.float64(10), TypeError), ("10", TypeError), (None, TypeError), (0, ValueError),
                                     (-3, ValueError), (np.int32(0), ValueError)])
def test_budget_must_be_a_positive_integer(bad, err):
    with pytest.raises(err):
        bs.check_budget(bad)
    with pytest.raises(err):
        bs.smallest_rate_within({1.0: 5}, bad)
    assert bs.check_budget(7) == 7 and bs.check_budget(np.uint64(7)) == 7


def test_sizes_entry_point_checks_its_arguments_before_the_device():
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    assert h.vbq_rans_sizes_u16(None, 1, 10, 11, 8, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert h.vbq_rans_sizes_u16(None, 1, 10, 10, 0, None, None, None) == -1
    assert h.vbq_rans_sizes_u16(None, 1, 10, 10, 65534, None, None, None) == -1
    assert h.vbq_rans_sizes_u16(None, 65536, 10, 10, 8, None, None, None) == -1
    assert h.vbq_rans_sizes_u16(None, -1, 10, 10, 8, None, None, None) == -1
    assert h.vbq_rans_sizes_u16(None, 2, 10, 10, 8, None, None, None) == -1 and b"null pointer" in h.vbq_last_error()
    assert h.vbq_rans_sizes_u16(None, 0, 10, 10, 8, None, None, None) == 0                 # nothing to do
    assert h.vbq_rans_sizes_u16(None, 3, 0, 10, 8, None, None, None) == 0


def test_segment_entry_points_share_their_size_checks():
    """The six entry points over (n_streams, n, N, seg) refuse alike, each under its own name, before any pointer is followed:
    bad sizes, and more segments per stream than the kernels' int holds -- the encoder and the decoder too, which once cast that
    count unchecked."""
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    p = 4096                                                     # a non-null pointer that is never followed
    calls = {
        "vbq_rans_encode_u16": lambda n, N, q=p: h.vbq_rans_encode_u16(p, 1, n, N, 1, p, p, q, None),
        "vbq_rans_sizes_u16": lambda n, N, q=p: h.vbq_rans_sizes_u16(p, 1, n, N, 1, p, q, None),
        "vbq_rans_decode_u16": lambda n, N, q=p: h.vbq_rans_decode_u16(p, p, 1, n, N, 1, p, q, None, None),
        "vbq_rans_map_encode_u16": lambda n, N, q=p: h.vbq_rans_map_encode_u16(p, 1, p, 1, 1, n, N, 1, p, p, q, None),
        "vbq_rans_map_sizes_u16": lambda n, N, q=p: h.vbq_rans_map_sizes_u16(p, 1, p, 1, 1, n, N, 1, p, q, None),
        "vbq_rans_map_decode_u16": lambda n, N, q=p: h.vbq_rans_map_decode_u16(p, p, p, 1, 1, n, N, 1, p, q, None, None),
    }
    for name, call in calls.items():
        assert call(10, 11) == -1
        assert h.vbq_last_error().startswith(name.encode() + b": bad sizes n_streams=1 n=10 N=11 seg=1"), name
        assert call(2 ** 31 + 1, 10) == -1
        assert h.vbq_last_error() == name.encode() + b": 2147483649 segments per stream are too many", name
        assert call(2 ** 31 - 1, 10, None) == -1                 # 2^31 - 1 segments pass the checks: on to the pointers
        assert h.vbq_last_error() == name.encode() + b": null pointer argument", name
