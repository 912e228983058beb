"""A public call of the quantizer that raises leaves it answering every probe exactly as it did before the call
(tests/quantizer_histories.py: FAILED_ATTEMPTS, the probes and the fresh oracle; the class docstring states the rule).

a. one test per attempt and state: fresh(state), every probe once (warm), the attempt -- which must raise its listed type --,
   then every probe again: each answer is the fresh quantizer's;
b. one chain: every attempt in a row on one quantizer, then every probe;
c. the control: a half-applied transition planted by hand -- raw_code_length_entropy_models = None beside the old models;
   the host tables of another state beside the old device cache -- changes at least one probe.
After a. and b. a copy of the quantizer without its caches (pickling) is asked the host-side probes too: a warm quantizer
answers from device copies made before the attempt, the copy from the host tables the attempt may have left behind.

States A (a strict table) and E (repeated code points: the models live on the host), the shapes of the harness.  Every
comparison is exact."""
import gc
import pickle
import time

import pytest

torch = pytest.importorskip("torch")

import quantizer_histories as QH  # noqa: E402
from test_gpu_quantizer_histories import disagreements, files_of, inputs, warm  # noqa: E402

pytestmark = pytest.mark.gpu
STATES = ("A", "E")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    t0 = time.perf_counter()
    yield
    print(f"\n[test_gpu_failed_calls] {time.perf_counter() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _drop_the_quantizer():
    """Every test builds a quantizer of its own, with captured graphs and their streams: collected when the test ends, not
    whenever the next cyclic collection happens to run."""
    yield
    gc.collect()


def attempt_inputs(state):
    """The inputs of the state, with the files a fresh quantizer of the OTHER state wrote for the readers that are given one."""
    inp = inputs(state)._copy()
    inp.foreign = files_of(QH.OTHER_STATE[state])
    return inp


def fail(q, name, inp):
    """The attempt raises exactly its listed type -- not a subclass, not something else on the way there."""
    fn, exc = QH.FAILED_ATTEMPTS[name]
    exc = QH.expected_type(exc)
    try:
        fn(q, inp)
    except Exception as e:                              # noqa: BLE001 -- the type is what is asserted
        assert type(e) is exc, f"{name}: raised {type(e).__name__}({str(e)[:200]!r}), expected {exc.__name__}"
        return
    raise AssertionError(f"{name}: the call did not raise (expected {exc.__name__})")


HOST_SIDE = ("intervals", "latents", "to_bytes", "r_decompress_b")
"""Probes whose answers come from the host tables build_code_points stores (the level-major table, the sorted one and the digest
of the code points) once no cached device copy stands in for them."""


def copy_without_caches(q):
    """What pickling gives: the quantizer's host state, none of its caches.  A warm quantizer answers from device copies made
    before the attempt, so host tables a failed build_code_points left behind would show only when a copy is made anew --
    after an eviction, in another process.  The pickled copy is that moment, reached without touching q._dev_cache."""
    return pickle.loads(pickle.dumps(q))


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", list(QH.FAILED_ATTEMPTS))
def test_failed_attempt_leaves_every_answer_as_it_was(name, state):
    q = QH.fresh(QH.STATES[state])
    warm(q, state)
    fail(q, name, attempt_inputs(state))
    bad = disagreements(q, state, inputs(state))
    assert not bad, f"after the failed {name} in state {state}: " + "; ".join(bad)
    bad = disagreements(copy_without_caches(q), state, inputs(state), only=HOST_SIDE)
    assert not bad, f"after the failed {name} in state {state}, a copy without the caches: " + "; ".join(bad)


@pytest.mark.parametrize("state", STATES)
def test_chain_of_failed_attempts(state):
    q = QH.fresh(QH.STATES[state])
    warm(q, state)
    inp = attempt_inputs(state)
    for name in QH.FAILED_ATTEMPTS:
        fail(q, name, inp)
    warm(q, state)
    bad = disagreements(copy_without_caches(q), state, inputs(state), only=HOST_SIDE)
    assert not bad, "a copy without the caches: " + "; ".join(bad)


def test_control_a_half_applied_transition_is_seen():
    """The probes can see what the attempts must not leave behind.  Planted by hand on a warm quantizer:
    raw_code_length_entropy_models = None beside the old entropy_models (the next solve takes raw lengths): the `latents` probe
    disagrees; code_points_by_channel of state E beside the old all_code_points, _strict and an untouched _dev_cache: the
    host-side probes of a copy without the caches disagree."""
    q = QH.fresh(QH.STATES["A"])
    warm(q, "A")
    saved = q.raw_code_length_entropy_models
    q.raw_code_length_entropy_models = None
    bad = disagreements(q, "A", inputs("A"), only=("latents",))
    assert bad, "raw_code_length_entropy_models = None beside the old models changed no answer of `latents`"
    q.raw_code_length_entropy_models = saved
    assert not disagreements(q, "A", inputs("A"), only=("latents",))
    assert not disagreements(copy_without_caches(q), "A", inputs("A"), only=HOST_SIDE)

    e = QH.fresh(QH.STATES["E"])
    assert q.code_points_by_channel.shape == e.code_points_by_channel.shape
    assert q.code_points_by_channel.tobytes() != e.code_points_by_channel.tobytes()
    cache_before = dict(q._dev_cache)
    q.code_points_by_channel = e.code_points_by_channel
    assert q._dev_cache.keys() == cache_before.keys() and all(q._dev_cache[k] is v for k, v in cache_before.items())
    bad = disagreements(copy_without_caches(q), "A", inputs("A"), only=HOST_SIDE)
    assert bad, f"code_points_by_channel of state E beside the old tables changed none of {HOST_SIDE}"
