"""The footprint helper can fail, and its coverage tables name every function of include/vbq.h (no GPU needed).

Control: on CPU tensors one planted byte is reported at its right offset -- directly before and after the payload, in the last
guard byte on either side, and inside the payload but outside a mask -- for every dtype and both byte canaries; an untouched
buffer passes.  Coverage: every declared function is in exactly one of footprint.COVERED and footprint.EXEMPT, every test
COVERED names exists in tests/test_gpu_write_footprint.py, and EXEMPT holds only the reasons the closed set allows, each for
the kind of entry point it is meant for."""
import ast
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import footprint as FP  # noqa: E402
from test_abi import declared_functions  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [torch.uint8, torch.uint16, torch.int32, torch.uint32, torch.int64, torch.uint64, torch.float32, torch.float64]
CASES = [(dt, u8) for dt in DTYPES for u8 in (FP.U8_CANARIES if dt == torch.uint8 else FP.U8_CANARIES[:1])]


def _plant(g, raw_offset):
    """Flip one byte of the allocation to a value it does not hold."""
    g.raw[raw_offset] = int(g.raw[raw_offset]) ^ 0xFF
    return int(g.raw[raw_offset])


@pytest.mark.parametrize("dtype,u8", CASES)
@pytest.mark.parametrize("offset_elems", [0, 1])
def test_canaries_and_layout(dtype, u8, offset_elems):
    g = FP.Guarded((3, 5), dtype, "cpu", offset_elems, 1024, u8)
    size = g.itemsize
    want = {torch.uint16: 0xABCD, torch.uint32: 0xA5C3E1D2, torch.int32: 0xA5C3E1D2, torch.int64: 0xA5C3E1D2A5C3E1D2,
            torch.uint64: 0xA5C3E1D2A5C3E1D2, torch.float32: 0x7FA5C3E1, torch.float64: 0x7FF4A5C3E1D2B697, torch.uint8: u8}[dtype]
    assert FP.canary(dtype, u8) == want and np.all(g.bits() == want)
    if dtype in (torch.float32, torch.float64):
        assert np.all(np.isnan(g.host()))                        # NaN payloads: compared through integer views only
    assert tuple(g.view.shape) == (3, 5) and g.view.dtype == dtype and g.view.is_contiguous()
    assert (g.view.data_ptr() - offset_elems * size) % 256 == 0 and g.view.data_ptr() == g.ptr
    assert g.lead == 1024 + offset_elems * size and g.trail == 1024
    g.assert_untouched("untouched")                                # an untouched buffer passes
    g.fill(np.arange(15).reshape(3, 5))
    assert np.array_equal(g.host(), np.arange(15).reshape(3, 5).astype(g.np_dtype))
    g.assert_outside_intact("filled")


@pytest.mark.parametrize("dtype,u8", CASES)
@pytest.mark.parametrize("offset_elems", [0, 1])
@pytest.mark.parametrize("where", ["directly before", "directly after", "first guard byte", "last guard byte"])
def test_a_planted_write_outside_is_reported_at_its_offset(dtype, u8, offset_elems, where):
    g = FP.Guarded((3, 5), dtype, "cpu", offset_elems, 1024, u8)
    at = {"directly before": -1, "directly after": g.nbytes, "first guard byte": -g.lead,
          "last guard byte": g.nbytes + g.trail - 1}[where]
    value = _plant(g, g.start + at)
    with pytest.raises(AssertionError) as e:
        g.assert_outside_intact("planted")
    assert re.search(rf"byte offset {at} relative to the payload .* holds 0x{value:02x}; 1 guard bytes damaged", str(e.value))
    g.assert_only(np.zeros((3, 5), bool))                          # the payload itself is still canary


@pytest.mark.parametrize("dtype,u8", CASES)
def test_a_planted_write_inside_but_outside_the_mask_is_reported(dtype, u8):
    g = FP.Guarded((3, 5), dtype, "cpu", 1, 1024, u8)
    mask = np.zeros((3, 5), bool)
    mask[1, 1:4] = True
    g.raw[g.start + (1 * 5 + 2) * g.itemsize] ^= 0xFF                 # inside the mask: allowed
    g.assert_only(mask, "inside the mask")
    _plant(g, g.start + (2 * 5 + 4) * g.itemsize + g.itemsize - 1)    # the last byte of element (2, 4)
    with pytest.raises(AssertionError, match=r"element \(2, 4\) of .* 1 elements damaged"):
        g.assert_only(mask, "planted")
    g.assert_outside_intact("the guards are intact")
    with pytest.raises(AssertionError, match="element"):
        g.assert_untouched("planted")


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 4100])
def test_workspace_guard(nbytes, u8):
    ws = FP.guarded_workspace(nbytes, "cpu", 256, u8)
    assert ws.view.dtype == torch.uint8 and ws.view.numel() == nbytes == ws.nbytes and ws.ptr % 256 == 0
    ws.assert_outside_intact("untouched")
    value = _plant(ws, ws.start + nbytes)                            # one byte past the size the library asked for
    with pytest.raises(AssertionError, match=rf"byte offset {nbytes} relative .* holds 0x{value:02x}"):
        ws.assert_outside_intact("planted")


def test_shifted_inputs_keep_their_values():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    for off in (0, 1):
        t = FP.shifted(a, off, "cpu")
        assert (t.data_ptr() - 4 * off) % 256 == 0 and t.is_contiguous() and np.array_equal(t.numpy(), a)


# ------------------------------------------------------------------------------------------------------------------ coverage
def _gpu_module_tests():
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_write_footprint.py")).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_declared_function_is_covered_or_exempt():
    declared = set(declared_functions())
    covered, exempt = set(FP.COVERED), set(FP.EXEMPT)
    assert not covered & exempt, sorted(covered & exempt)
    assert covered | exempt == declared, (sorted(declared - covered - exempt), sorted((covered | exempt) - declared))


def test_every_named_test_exists_and_every_test_is_named():
    have = _gpu_module_tests()
    named = {t for tests in FP.COVERED.values() for t in tests}
    assert all(tests for tests in FP.COVERED.values())
    assert named <= have, sorted(named - have)
    assert have <= named, sorted(have - named)                     # no test of the module guards nothing the table knows of


def test_exemptions_hold_only_the_allowed_reasons():
    queries = {"vbq_abi_version", "vbq_last_error", "vbq_solve_grid", "vbq_device_count", "vbq_device_name", "vbq_records_words"}
    for name, reason in FP.EXEMPT.items():
        if reason == FP.NO_WRITE:
            assert name in queries or name.endswith("_workspace_bytes"), name
        elif reason == FP.HOST:
            assert name.startswith("vbq_host_"), name
        elif reason == FP.COMM:
            assert name.startswith("vbq_comm_") or name == "vbq_allreduce_hist", name
        elif reason.startswith(FP.UNTOUCHED):
            assert name.endswith("_files_u16") or name.endswith("_window_f32"), name
            module, test = reason[len(FP.UNTOUCHED):].split("::")
            tree = ast.parse(open(os.path.join(HERE, module + ".py")).read())
            assert test in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, reason
        else:
            pytest.fail(f"{name}: {reason!r} is not an allowed reason for an entry point")
    assert set(FP.EXEMPT_INSTANCES.values()) <= {FP.TOO_LARGE} and list(FP.EXEMPT_INSTANCES) == ["k_quant_hull_idx<BUF = false>"]
