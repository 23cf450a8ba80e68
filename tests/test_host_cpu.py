"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol of include/scp_hip.h
(no compute calls without a GPU), the product path fails loudly without a GPU, scenario generators match the
reference's fixtures, the batch CLI keeps the reference's output schema, and the oracle's QP solvers agree with
each other and with an independent optimiser."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scp_hip.h")


def header_text():
    """include/scp_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def header_structs(text):
    """{struct name: [field names in order]} of every `typedef struct scp_x { ... } scp_x;` with a body"""
    out = {}
    for name, body in re.findall(r"^typedef struct (scp_\w+)\s*\{(.*?)\}\s*\w+\s*;", text, flags=re.M | re.S):
        out[name] = [re.match(r"\w+", d.strip()).group(0)  # `double r_prim, r_dual;` declares two, `added[N]` is `added`
                     for decl in body.split(";") if decl.strip()
                     for d in decl.strip().split(None, 1)[1].split(",")]
    return out


def header_functions(text):
    """{function: (return type, [parameter types])} of every declaration that starts in column 0 and ends in `);`, as C
    type strings without `const` and blanks (`double*`, `scp_ctx**`, `int`); the static inline helper is no declaration"""
    def ctype(s):
        return re.sub(r"\bconst\b|\s+", "", s)

    out = {}
    for ret, name, params in re.findall(r"^(?!typedef|static)(\w[\w \*]*?)\b(scp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.M):
        params = [p.strip() for p in params.split(",")]
        out[name] = (ctype(ret), [] if params == ["void"] else [ctype(re.sub(r"\w+$", "", p)) for p in params])
    return out


C_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
             **{f"{u}int{b}_t": getattr(ctypes, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
OPAQUE = ("void", "scp_ctx", "scp_qp", "scp_solver")  # handles and untyped addresses


def scalar_class(ct):
    """(kind, bytes) of a ctypes scalar: c_size_t and c_uint64 are one class where they are one type"""
    code = ct._type_
    return ("f" if code in "fd" else "u" if code.isupper() else "i"), ctypes.sizeof(ct)


def type_mismatch(c, ct, structs):
    """why the ctypes type `ct` of a table row does not fit the C type `c` of the header (None: it fits)"""
    if c == "void" or ct is None:
        return None if (c == "void" and ct is None) else f"{c} against {ct}"
    if c == "char*":
        return None if ct is ctypes.c_char_p else f"const char* against {ct}"
    if not c.endswith("*"):
        ok = isinstance(ct, type) and issubclass(ct, ctypes._SimpleCData) and ct not in (ctypes.c_void_p, ctypes.c_char_p)
        return None if ok and scalar_class(ct) == scalar_class(C_SCALARS[c]) else f"{c} against {ct}"
    pointee = c[:-1]
    if ct is ctypes.c_void_p:  # an opaque handle or a device address
        return f"{c} against c_void_p" if pointee.endswith("*") else None
    if not (isinstance(ct, type) and issubclass(ct, ctypes._Pointer)):
        return f"{c} against {ct}"
    to = ct._type_
    if pointee.endswith("*"):
        return None if to is ctypes.c_void_p else f"{c} against a pointer to {to}"
    if pointee in structs:
        return None if to is structs[pointee] else f"{c} against a pointer to {to}"
    if pointee in OPAQUE:
        return f"{c} is opaque: c_void_p, not a pointer to {to}"
    ok = issubclass(to, ctypes._SimpleCData) and scalar_class(to) == scalar_class(C_SCALARS[pointee])
    return None if ok else f"{c} against a pointer to {to}"


def prototype_errors(table, structs, declared):
    """every disagreement between a prototype table (name -> (restype, argtypes)) and the header's declarations"""
    errors = [f"{n}: declared in the header, no row in the table" for n in declared if n not in table]
    errors += [f"{n}: a row in the table, not declared in the header" for n in table if n not in declared]
    for name in sorted(set(table) & set(declared)):
        (restype, argtypes), (ret, params) = table[name], declared[name]
        why = type_mismatch(ret, restype, structs)
        if why:
            errors.append(f"{name}: return type {why}")
        if len(argtypes) != len(params):
            errors.append(f"{name}: {len(argtypes)} argtypes for {len(params)} parameters")
            continue
        for i, (c, ct) in enumerate(zip(params, argtypes)):
            why = type_mismatch(c, ct, structs)
            if why:
                errors.append(f"{name}: parameter {i} {why}")
    return errors


def c_layouts(structs, tmp_path):
    """{struct: (sizeof, {field: (offsetof, sizeof)})} as gcc sees include/scp_hip.h, for the fields the mirrors name (a
    field the header lacks does not compile), and SCP_ABI_VERSION"""
    import subprocess

    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "scp_hip.h"', "int main(void) {"]
    for name, cls in structs.items():
        src.append(f'  printf("{name} %zu", sizeof({name}));')
        src += [f'  printf(" {f} %zu %zu", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, *_ in cls._fields_]
        src.append('  printf("\\n");')
    src.append('  printf("abi %d\\n", SCP_ABI_VERSION);\n  return 0; }')
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    out = {}
    for words in map(str.split, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()):
        rest = words[2:]
        out[words[0]] = (int(words[1]), {rest[i]: (int(rest[i + 1]), int(rest[i + 2])) for i in range(0, len(rest), 3)})
    return out, out.pop("abi")[0]


def struct_errors(structs, layouts, declared):
    """every disagreement between the mirrors (C struct name -> ctypes Structure), the C compiler's layouts and the field
    lists of the header"""
    errors = [f"{n}: a struct of the header without a mirror" for n in declared if n not in structs]
    for name, cls in structs.items():
        fields = [f for f, *_ in cls._fields_]
        if name not in declared or name not in layouts:
            errors.append(f"{name}: a mirror of no struct of the header")
            continue
        if fields != declared[name]:
            errors.append(f"{name}: fields {fields}, the header declares {declared[name]}")
        size, at = layouts[name]
        if ctypes.sizeof(cls) != size:
            errors.append(f"{name}: {ctypes.sizeof(cls)} bytes, {size} in C")
        for f in fields:
            got = (getattr(cls, f).offset, getattr(cls, f).size)
            if f in at and got != at[f]:
                errors.append(f"{name}.{f}: (offset, size) {got}, {at[f]} in C")
    return errors


def test_library_exports_every_declared_symbol():
    from path_planning import _hip

    path = _hip.library_path()
    assert os.path.exists(path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(path)
    declared = set(re.findall(r"\b(scp_[a-z0-9_]+)\s*\(", header_text())) - {"scp_eta_stride"}  # static inline helper
    assert declared == set(_hip.EXPORTS) == set(_hip.PROTOTYPES), declared ^ set(_hip.EXPORTS)
    assert len(_hip.EXPORTS) == len(set(_hip.EXPORTS))
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.scp_abi_version() == _hip.ABI_VERSION == int(re.search(r"#define SCP_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    s = _hip.default_settings()
    assert (s.rho, s.sigma, s.alpha, s.eps_abs, s.eps_rel, s.max_iter, s.check_termination) == (
        0.1, 1e-6, 1.6, 1e-3, 1e-3, 4000, 25)  # OSQP defaults


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from path_planning import _hip
    from path_planning.solvers.scp import SCP

    with pytest.raises(_hip.HipError, match="no GPU"):
        SCP(n_vehicles=2, time_horizon=1.0, time_step=0.2, min_distance=0.5, verbose=False)


def test_scp_bases_do_not_shadow_each_other():
    """SCP is one class assembled from state-free bases: a method name defined in two of them (or in a base and in SCP itself)
    would silently hide one definition, and a base with an __init__ would run instead of, or be hidden by, SCP's."""
    from path_planning.solvers.scp import SCP

    bases = SCP.__bases__
    assert [b.__name__ for b in bases] == ["ObstacleMethods", "ValidationMethods", "FleetMethods"]
    owners = {}
    for cls in (SCP,) + bases:
        for name in vars(cls):
            if not (name.startswith("__") and name.endswith("__")) or name == "__init__":
                owners.setdefault(name, []).append(cls.__name__)
    assert {n: o for n, o in owners.items() if len(o) > 1} == {}
    assert owners["__init__"] == ["SCP"]
    for b in bases:
        assert b.__bases__ == (object,)
        assert not [n for n, v in vars(b).items() if not n.startswith("__") and not callable(v) and not isinstance(v, staticmethod)]


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "ba-path-planning_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, os.path.join(dirpath, f)


def test_generator_matches_reference_fixture(golden_dir):
    import random

    from path_planning.scenarios.position_generator import generate_positions

    g = np.load(os.path.join(golden_dir, "ref_generator.npz"))
    for n, s, md in ((4, 1, 0.8), (10, 7, 0.8), (20, 20, 0.8), (50, 3, 0.8), (20, 5, 1.0)):
        a, b = generate_positions(n, md, seed=s)
        np.testing.assert_array_equal(a, g[f"init_n{n}_s{s}_d{md}"])
        np.testing.assert_array_equal(b, g[f"final_n{n}_s{s}_d{md}"])
        random.seed(s)  # the reference's own way: global random module
        a2, b2 = generate_positions(n, md)
        np.testing.assert_array_equal(a, a2)
    assert bool(g["n80_raises"])
    with pytest.raises(ValueError, match=str(g["n80_message"])):
        generate_positions(80, 0.8, seed=0)


def test_grid_swap_scenarios():
    from path_planning.scenarios.position_generator import generate_grid_swap, straight_line_min_distance

    for n, dim in ((64, 2), (64, 3), (100, 2)):
        a, b, space = generate_grid_swap(n, seed=1000 * n, dim=dim)
        assert a.shape == b.shape == (n, dim) and len(space) == 2 * dim
        a2, b2, _ = generate_grid_swap(n, seed=1000 * n, dim=dim)
        np.testing.assert_array_equal(a, a2)  # seeded
        d0 = np.linalg.norm(a[:, None] - a[None], axis=2) + 10 * np.eye(n)
        assert d0.min() > 0.8 and (np.linalg.norm(b[:, None] - b[None], axis=2) + 10 * np.eye(n)).min() > 0.8
        assert np.linalg.norm(a - b, axis=1).max() < 10.0  # reachable with |v| <= 2 in T = 10
        assert straight_line_min_distance(a, b).min() > 0.1  # no head-on swaps
        assert (a >= np.array(space[:dim])).all() and (b <= np.array(space[dim:])).all()


def test_batch_cli_schema(tmp_path, monkeypatch):
    """JSON/CSV schema of compute_trajectories_batch.py:91-100, :158 (solver stubbed: no GPU here)."""
    import csv
    import json

    from path_planning.cli import compute_trajectories_batch as cli

    def fake_trial(N, cfg, rng=None, seed=None, device=None, scenario=None, save_path=None, pool=None):
        assert scenario is not None and scenario[0].shape == (N, 2)  # generated before the timed loop
        return {"N": N, "status": "success" if seed % 2 == 0 else "error", "time_sec": 0.1 * N + 0.01 * (seed % 7),
                "error": None if seed % 2 == 0 else "boom", "K": 50, "T": cfg["time_horizon"], "h": cfg["time_step"],
                "seed": seed, "scp_iterations": 3}

    monkeypatch.setattr(cli, "run_single_trial", fake_trial)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res = cli.main(["--Ns", "4", "6", "--trials", "3", "--seed", "10", "--results-dir", str(tmp_path)])
    assert set(res) == {"meta", "runs", "summary"} and res["meta"]["schema_version"] == "1.0"
    assert len(res["runs"]) == 6 and [r["trial_index"] for r in res["runs"]] == [0, 1, 2, 0, 1, 2]
    assert res["runs"][0]["seed"] == 10 + 1000 * 4 + 0  # rng_seed + 1000*N + trial (:108)
    s4 = res["summary"]["4"]
    assert set(s4) == {"count", "errors", "min", "max", "mean", "median", "p25", "p75", "std"}
    assert s4["count"] + s4["errors"] == 3
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 2 and files[0].endswith(".csv") and files[1].endswith(".json")
    rows = list(csv.reader(open(tmp_path / files[0])))
    assert rows[0] == ["N", "trial_index", "status", "time_sec", "K", "T", "h", "error"] and len(rows) == 7
    assert json.load(open(tmp_path / files[1]))["summary"].keys() == {"4", "6"}
    # scenario-parallel job split: every job on exactly one rank
    cfg = dict(cli.CONFIG, Ns=[4, 6], trials_per_N=3)
    jobs = [cli.jobs_for_rank(cfg, r, 4) for r in range(4)]
    assert sorted(j for part in jobs for j in part) == [(n, t) for n in (4, 6) for t in range(3)]


def test_qp_oracles_agree_and_match_trust_constr():
    """QP#0 of the N=4, K=20 plumbing case: structured ADMM == explicit OSQP restatement == scipy trust-constr
    == closed-form min-norm solution (no box row is active there)."""
    from scipy.optimize import LinearConstraint, minimize

    from oracle import qp_oracle as qo
    from oracle import scp_oracle as so
    from path_planning.scenarios.position_generator import generate_positions

    p0, pf = generate_positions(4, 0.8, seed=1)
    prob = so.make_problem(4, 10.0, 0.5, 0.8, [0, 0, 20, 20], p0, pf)
    xs, _, info = qo.admm_structured(prob, st=qo.Settings(eps_abs=1e-9, eps_rel=1e-9))
    assert info["status_val"] == 1
    C, l, u = so.stack_fixed(prob)
    r = qo.osqp_explicit(2 * sp.eye(prob.n, format="csc"), np.zeros(prob.n), C, l, u, eps_abs=1e-9, eps_rel=1e-9,
                         max_iter=20000)
    assert r["status_val"] == 1
    np.testing.assert_allclose(xs.ravel(), r["x"], rtol=0, atol=1e-7)
    # closed form: min ||x||^2 s.t. E x = e (the two equality rows per agent/axis)
    eq = np.nonzero(l == u)[0]
    E = C.tocsr()[eq].toarray()
    x_mn = E.T @ np.linalg.solve(E @ E.T, l[eq])
    assert np.all(C @ x_mn >= l - 1e-9) and np.all(C @ x_mn <= u + 1e-9)
    np.testing.assert_allclose(xs.ravel(), x_mn, rtol=0, atol=1e-7)
    # independent optimiser on a smaller instance (trust-constr is slow on dense 160-variable problems)
    prob2 = so.make_problem(2, 5.0, 0.5, 0.8, [0, 0, 20, 20], p0[:2], pf[:2] * 0.5 + p0[:2] * 0.5)
    C2, l2, u2 = so.stack_fixed(prob2)
    x2, _, i2 = qo.admm_structured(prob2, st=qo.Settings(eps_abs=1e-9, eps_rel=1e-9))
    assert i2["status_val"] == 1
    res = minimize(lambda x: x @ x, np.zeros(prob2.n), jac=lambda x: 2 * x, hess=lambda x: 2 * np.eye(prob2.n),
                   constraints=[LinearConstraint(C2.toarray(), l2, u2)], method="trust-constr",
                   options={"gtol": 1e-12, "xtol": 1e-14, "maxiter": 300})
    np.testing.assert_allclose(res.x, x2.ravel(), rtol=0, atol=1e-6)


def test_structured_vs_explicit_collision_qp():
    """Joint QP with collision rows: constraint generation (working set) reaches the optimum of the FULL QP."""
    from oracle import qp_oracle as qo
    from oracle import scp_oracle as so
    from path_planning.scenarios.position_generator import generate_positions

    p0, pf = generate_positions(4, 0.8, seed=1)
    prob = so.make_problem(4, 10.0, 0.5, 0.8, [0, 0, 20, 20], p0, pf)
    x0, _, _ = qo.admm_structured(prob, st=qo.Settings(eps_abs=1e-9, eps_rel=1e-9))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    xs, _, info = qo.admm_structured(prob, eta, l_col, dist, x0=x0,
                                     st=qo.Settings(eps_abs=1e-9, eps_rel=1e-9, max_iter=50000, margin=0.05))
    assert info["status_val"] == 1 and info["working_rows"] < prob.m_col
    C, lf, uf = so.stack_fixed(prob)
    A = sp.vstack([C, so.collision_matrix_explicit(prob, eta)], format="csc")
    r = qo.osqp_explicit(2 * sp.eye(prob.n, format="csc"), np.zeros(prob.n), A, np.hstack([lf, l_col]),
                         np.hstack([uf, np.full(l_col.size, np.inf)]), x0=x0.ravel(), eps_abs=1e-10, eps_rel=1e-10,
                         max_iter=200000)
    assert r["status_val"] == 1
    np.testing.assert_allclose(xs.ravel(), r["x"], rtol=0, atol=1e-6)
    assert np.all(A @ xs.ravel() >= np.hstack([lf, l_col]) - 1e-6)


def test_graft_entry_build_runs_on_cpu():
    """The driver's "does it build" check: __graft_entry__.build() compiles libscp_hip.so for gfx950 and the oracle's C
    restatement (incremental: a no-op after the first build), imports the package and checks exports + ABI version."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    g.build()


HOST_STRUCTS = ("scp_qp_settings", "scp_qp_info", "scp_pair_stats", "scp_solve_options", "scp_qp_record", "scp_solve_result")


def test_ctypes_structs_match_the_header(tmp_path):
    """Every struct of include/scp_hip.h has a ctypes mirror in _hip.STRUCTS, and every mirror has the size, the field names
    and, for every field, the offset and the size that gcc gives the C declaration; each numpy dtype derives from its mirror."""
    from path_planning import _hip

    declared = header_structs(header_text())
    assert sorted(declared) == sorted(re.findall(r"typedef struct (scp_\w+)\s*\{", header_text())), "the parser lost a struct"
    assert set(HOST_STRUCTS) <= set(declared), sorted(declared)
    layouts, abi = c_layouts(_hip.STRUCTS, tmp_path)
    assert struct_errors(_hip.STRUCTS, layouts, declared) == []
    for name in HOST_STRUCTS:  # (spelled out: the sizes of the six structs the host reads or writes)
        assert ctypes.sizeof(_hip.STRUCTS[name]) == layouts[name][0], name
    assert ctypes.sizeof(_hip.PairStats) == 32
    for name, value in vars(_hip).items():
        if name.endswith("_DTYPE"):
            mirror = [cls for cls in _hip.STRUCTS.values() if np.dtype(cls) == value]
            assert len(mirror) == 1 and value.itemsize == ctypes.sizeof(mirror[0]), name
    assert abi == _hip.ABI_VERSION
    assert _hip.pipeline_names(0) == "none" and _hip.pipeline_names((1 << 1) | (1 << 3)) == "persistent+three-launch"
    assert _hip.pipeline_names(1 << 7) == "persistent8-lean"


def test_prototypes_match_the_header():
    """Every function include/scp_hip.h declares has a row in _hip.PROTOTYPES and the reverse; arity, every parameter and the
    return type agree in class (scalars: kind and byte size; const char*: c_char_p; pointers: c_void_p for handles and device
    addresses, POINTER(Mirror) only for that very struct, POINTER(scalar) for a pointee of that kind and size)."""
    from path_planning import _hip

    declared = header_functions(header_text())
    named = set(re.findall(r"\b(scp_[a-z0-9_]+)\s*\(", header_text())) - {"scp_eta_stride"}  # (as the export test finds them)
    assert set(declared) == named, "the parser lost a declaration: " + str(set(declared) ^ named)
    assert prototype_errors(_hip.PROTOTYPES, _hip.STRUCTS, declared) == []


def test_abi_checks_report_broken_copies():
    """The two comparisons above find what they are there to find: wrong copies of the tables are reported by name.  Plain
    Python on copies: nothing is compiled, loaded or called (the layouts are those of the mirrors the test above holds to C)."""
    from path_planning import _hip

    text = header_text()
    declared, table = header_functions(text), dict(_hip.PROTOTYPES)

    def report(name, restype, argtypes):
        return prototype_errors(dict(table, **{name: (restype, argtypes)}), _hip.STRUCTS, declared)

    res, args = table["scp_list_conflicts"]
    i = args.index(ctypes.c_int64)
    narrow = report("scp_list_conflicts", res, args[:i] + [ctypes.c_int32] + args[i + 1:])  # an i32 where C takes int64_t
    assert len(narrow) == 1 and narrow[0].startswith(f"scp_list_conflicts: parameter {i} int64_t"), narrow
    dropped = report("scp_list_conflicts", res, args[:i] + args[i + 1:])
    assert dropped == [f"scp_list_conflicts: {len(args) - 1} argtypes for {len(args)} parameters"], dropped
    assert table["scp_ctx_destroy"][0] is None
    default = report("scp_ctx_destroy", ctypes.c_int, table["scp_ctx_destroy"][1])  # restype left at ctypes' default
    assert default == [f"scp_ctx_destroy: return type void against {ctypes.c_int}"], default
    missing = prototype_errors({k: v for k, v in table.items() if k != "scp_abi_version"}, _hip.STRUCTS, declared)
    assert missing == ["scp_abi_version: declared in the header, no row in the table"], missing
    other = report("scp_qp_solve", res, [ctypes.c_void_p, ctypes.POINTER(_hip.QpRecord)])  # a pointer to the wrong struct
    assert len(other) == 1 and other[0].startswith("scp_qp_solve: parameter 1 scp_qp_info*"), other

    good = _hip.Conflict._fields_

    class Swapped(ctypes.Structure):  # scp_conflict with min_dist and t_min exchanged: the same size, the same field set
        _fields_ = [good[0], good[2], good[1], *good[3:]]

    layouts = {name: (ctypes.sizeof(cls), {f: (getattr(cls, f).offset, getattr(cls, f).size) for f, *_ in cls._fields_})
               for name, cls in _hip.STRUCTS.items()}
    found = struct_errors(dict(_hip.STRUCTS, scp_conflict=Swapped), layouts, header_structs(text))
    assert len(found) == 3 and found[0].startswith("scp_conflict: fields ['row', 't_min', 'min_dist'"), found
    assert [e.split(":")[0] for e in found[1:]] == ["scp_conflict.t_min", "scp_conflict.min_dist"], found
