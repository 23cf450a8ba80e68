"""CPU-only checks of the table of tests/ctx_state_cases.py: every entry point that launches on a context has a case or a
stated exemption, every case's reference satisfies the case's own criterion and is deterministic, and every family's grower
leaves each shared buffer larger than any case of the family needs."""
import numpy as np
import pytest

import ctx_state_cases as cs
from test_host_cpu import header_functions, header_text


def launching_entry_points():
    """the functions of include/scp_hip.h whose first parameter is a context, a QP or a solver handle: all of them work on a
    context's stream and may touch what it owns"""
    out = []
    for name, (_, params) in header_functions(header_text()).items():
        if params and params[0] in ("scp_ctx*", "scp_qp*", "scp_solver*"):
            out.append(name)
    return out


def test_every_entry_point_has_a_case_or_an_exemption():
    from path_planning import _hip

    names = launching_entry_points()
    assert set(names) <= set(_hip.PROTOTYPES) and len(names) > 60
    covered = {e for c in cs.CASES for e in c.entries}
    assert covered <= set(_hip.PROTOTYPES), covered - set(_hip.PROTOTYPES)
    # (scp_qp_create and scp_solver_create take the context first: they are in `names` already)
    missing = [n for n in names if n not in covered and n not in cs.EXEMPT]
    assert not missing, f"entry points without a case in tests/ctx_state_cases.py and without an exemption: {missing}"
    both = sorted(covered & set(cs.EXEMPT))
    assert not both, f"exempt and covered at once: {both}"
    stale = sorted(set(cs.EXEMPT) - set(names))
    assert not stale, f"exemptions of functions the header does not declare: {stale}"
    for name, reason in cs.EXEMPT.items():
        assert reason.strip() and "\n" not in reason, name
        assert any(word in reason for word in ("lifecycle", "setter", "getter", "hook")), (name, reason)


def test_every_user_of_the_shared_workspace_is_in_both_orders():
    assert len(cs.SEP_WS_USERS) == 12 and sorted(cs.PRODUCT_ORDER) == sorted(cs.SEP_WS_USERS.values())
    for entry, name in cs.SEP_WS_USERS.items():
        case = cs.CASES_BY_NAME[name]
        assert entry in case.entries, (entry, name)
        assert case.ws()["sep_ws"][0] > 0, name  # the case does carve a layout from the workspace


def test_families_and_growers():
    assert {c.family for c in cs.CASES} == set(cs.FAMILIES) == set(cs.GROWERS)
    for family, grower in cs.GROWERS.items():
        assert grower.family == family and grower.reference is None


@pytest.mark.parametrize("name", list(cs.CASES_BY_NAME))
def test_reference_satisfies_the_cases_own_criterion_and_is_deterministic(name):
    case = cs.CASES_BY_NAME[name]
    inp = case.inputs()
    ref = case.ref()
    out = case.from_ref(ref, inp)
    case.compare(out, ref, inp)
    cs.assert_no_canary(out)
    again = case.from_ref(case.reference(inp), inp)  # a second evaluation, nothing cached
    cs.assert_same_bits(again, out, name)


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_grower_needs_strictly_more_of_every_shared_buffer(family):
    grown = cs.GROWERS[family].ws()
    for case in (c for c in cs.CASES if c.family == family):
        for buf, (low, high) in case.ws().items():
            assert low <= high
            if high > 0:
                assert buf in grown and grown[buf][0] > high, (case.name, buf, (low, high), grown.get(buf))


def test_same_bits_sees_one_bit():
    a = {"x": np.array([1.0, 2.0]), "n": 3, "f": 0.1, "d": {"m": np.arange(4, dtype=np.uint32)}}
    b = {"x": np.array([1.0, np.nextafter(2.0, 3.0)]), "n": 3, "f": 0.1, "d": {"m": np.arange(4, dtype=np.uint32)}}
    cs.assert_same_bits(a, a)
    for other in (b, dict(a, n=4), dict(a, f=np.nextafter(0.1, 1.0)), dict(a, x=a["x"].astype(np.float32)), {k: a[k] for k in ("x", "n", "f")}):
        with pytest.raises(AssertionError):
            cs.assert_same_bits(a, other)
    with pytest.raises(AssertionError):
        cs.assert_no_canary({"y": np.frombuffer(bytes([cs.CANARY] * 16), dtype=np.float64)})
    with pytest.raises(AssertionError):
        cs.assert_no_canary({"y": np.array([0, cs.CANARY, 1], dtype=np.uint8)})
