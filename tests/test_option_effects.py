"""What a call of hipfact_set_option does besides storing the value, option by option: which options drop the captured
graphs, which make the next set_matrix analyse again, on every call or only when the value changes, what the clamps
give, and which HIPFACT_* variables a new handle reads.  The smallest saddle problem there is (48 x 48): nothing here
depends on size.  Observables are info keys alone.  Every option of the header's table is in exactly one class below."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sleqp_amd import synth
from sleqp_amd._lib import HipfactError

gpu = pytest.mark.gpu

# name -> the value the test sets: the default of a new handle (a value that is NOT the default where nothing is
# invalidated whatever the value), and for the "on a change" classes the default and a second value
NO_INVALIDATION = {"refine_max": 7, "fail_omega": 1e-6, "static_pivot": 0, "debug_fake_timeout": 0, "cg_device_loop": 0,
                   "lz_device_loop": 0, "factor_hint_peek": 0, "top_block_breakeven": 7, "validate_rhs": 1, "spmv_stream": 0,
                   "spmv_stream_min": 1000, "assemble_superset": 0}
GRAPHS_ALWAYS = {"refine_steps": 1, "refine_adaptive": 1, "refine_tol": 1e-10, "static_pivot_delta": 1e-8, "equilibrate": 1}
GRAPHS_WHEN_OFF = {"use_graph": 1}
GRAPHS_ON_CHANGE = {"xupd_blocks": (256, 2), "cg_residual_update": (1, 0), "xupd_fused": (1, 0), "rhs_fused": (1, 0),
                    "decide_lazy": (1, 0)}
PLANS_ALWAYS = {"factor_top_max": 160, "pull_max_children": 4, "factor_top_levels": 1 << 20, "solve_fused": 1,
                "top_block_after": 2, "ordering": 0, "max_children": 4, "force_generic": 0, "dense_mode": 1}
PLANS_ON_CHANGE = {"solve_slices": (1, 0), "chain_pairs": (1, 0), "solve_sorted": (1, 0), "solve_whole_max": (48, 64),
                   "chain_fuse": (1, 0), "spanel_fold": (1, 0), "spanel_fold_room": (224, 100)}
# an action of their own and no invalidation (the default value of each)
OWN_ACTION = {"refine_check_backoff": 2, "refine_check_every": 8, "boundary_fast": 1, "boundary_profile": 0,
              "superset_vtable": 1, "exact_pattern": 0, "plan_cache": 4, "profile": 0}
CLASSES = (NO_INVALIDATION, GRAPHS_ALWAYS, GRAPHS_WHEN_OFF, GRAPHS_ON_CHANGE, PLANS_ALWAYS, PLANS_ON_CHANGE, OWN_ACTION)

PROF_CLASSES = ("memset", "mvals", "gather", "factor", "factorA", "factorB", "factorC", "factorD", "factorT", "fwd", "bwd",
                "rhs", "xupd", "resid", "axpy", "perm", "spanel", "tree")


def _problem(seed=1, n=36, m=12):
    from sleqp_amd.sparse import SleqpMat

    N, cp, ri, vx = synth.kkt_lower_from_jacobian(synth.banded_jacobian(n, m, 4, 12, seed))
    return SleqpMat(N, N, cp, ri, vx), np.random.default_rng(seed).standard_normal(N)


MAT, RHS = _problem()


@pytest.fixture
def fact():
    from sleqp_amd.fact import HipFact

    made = []

    def make(solves=2, **options):
        f = HipFact(device=0, **options)
        made.append(f)
        f.set_matrix(MAT)
        for _ in range(solves):
            f.solve(RHS)
        if solves:
            f.solution_raw(0, f.N)
        return f

    yield make
    for f in made:
        f.free()


def _solve_bits(f):
    f.solve(RHS)
    return f.solution_raw(0, f.N).view(np.uint64)


def _state(f):
    return f.info("num_graphs"), f.info("analyses")


@gpu
@pytest.mark.parametrize("name", list(GRAPHS_ALWAYS))
def test_drops_graphs_on_every_call(fact, name):
    f = fact()
    current = {"static_pivot_delta": 1e-8}.get(name)
    if current is None:
        current = f.info(name)
    assert current == GRAPHS_ALWAYS[name] and f.info("num_graphs") > 0
    f.set_option(name, current)
    assert f.info("num_graphs") == 0


@gpu
def test_use_graph_drops_graphs_only_when_switched_off(fact):
    f = fact()
    graphs = f.info("num_graphs")
    assert graphs > 0 and f.info("use_graph") == 1
    f.set_option("use_graph", 1)
    assert f.info("num_graphs") == graphs
    f.set_option("use_graph", 0)
    assert f.info("num_graphs") == 0 and f.info("use_graph") == 0
    _solve_bits(f)
    assert f.info("num_graphs") == 0


@gpu
@pytest.mark.parametrize("name", list(GRAPHS_ON_CHANGE))
def test_drops_graphs_only_on_a_change(fact, name):
    value, other = GRAPHS_ON_CHANGE[name]
    f = fact()
    before = _solve_bits(f)
    graphs, analyses = _state(f)
    assert graphs > 0
    f.set_option(name, value)
    assert _state(f) == (graphs, analyses)
    f.set_option(name, other)
    assert _state(f) == (0, analyses)
    f.set_option(name, value)
    assert np.array_equal(_solve_bits(f), before)
    f.set_matrix(MAT)
    assert f.info("analyses") == analyses


@gpu
@pytest.mark.parametrize("name", list(PLANS_ALWAYS))
def test_invalidates_plans_on_every_call(fact, name):
    f = fact()
    analyses = f.info("analyses")
    f.set_option(name, PLANS_ALWAYS[name])
    assert f.info("num_graphs") == 0
    f.set_matrix(MAT)
    assert f.info("analyses") == analyses + 1


@gpu
@pytest.mark.parametrize("name", list(PLANS_ON_CHANGE))
def test_invalidates_plans_only_on_a_change(fact, name):
    value, other = PLANS_ON_CHANGE[name]
    f = fact()
    graphs, analyses = _state(f)
    assert graphs > 0
    f.set_option(name, value)
    assert _state(f) == (graphs, analyses)
    f.set_matrix(MAT)
    assert f.info("analyses") == analyses
    f.set_option(name, other)
    assert f.info("num_graphs") == 0
    f.set_matrix(MAT)
    assert f.info("analyses") == analyses + 1


@gpu
@pytest.mark.parametrize("name", list(NO_INVALIDATION) + list(OWN_ACTION))
def test_leaves_graphs_and_plans_alone(fact, name):
    f = fact()
    graphs, analyses = _state(f)
    assert graphs > 0
    f.set_option(name, {**NO_INVALIDATION, **OWN_ACTION}[name])
    assert _state(f) == (graphs, analyses)
    f.set_matrix(MAT)
    assert f.info("analyses") == analyses


@gpu
def test_clamps(fact):
    f = fact()
    f.set_option("refine_steps", -3)
    assert f.info("refine_steps") == 0 and f.info("refine_inline") == 0
    f.set_option("refine_steps", 1)
    f.set_option("xupd_blocks", 0)
    f.set_option("refine_check_every", 0)
    assert f.info("refine_check_every") == 1
    f.set_matrix(MAT)
    f.solve(RHS)
    assert f.info("xupd_in_tree") == 1 and f.info("xupd_blocks_launched") >= 1
    assert f.info("refine_check_interval") >= 1


@gpu
@pytest.mark.parametrize("name", ["refine_check_every", "refine_check_backoff"])
def test_check_options_reset_the_interval_in_force(fact, name):
    f = fact()
    assert f.info("refine_check_interval") >= 1
    f.set_option(name, OWN_ACTION[name])
    assert f.info("refine_check_interval") == 0
    f.solve(RHS)
    assert f.info("refine_check_interval") >= 1


@gpu
def test_boundary_fast_reads_back(fact):
    f = fact()
    assert f.info("boundary_fast") == 1
    f.set_option("boundary_fast", 0)
    assert f.info("boundary_fast") == 0
    assert np.array_equal(_solve_bits(f), _solve_bits(f))


@gpu
def test_boundary_profile_counts_and_resets(fact):
    f = fact(boundary_profile=1)
    assert f.info("bd_count") >= 1
    f.set_option("boundary_profile", 1)
    assert f.info("bd_count") == 0


@gpu
@pytest.mark.parametrize("name", ["superset_vtable", "exact_pattern"])
def test_pattern_options_clear_the_row_dictionary_on_a_change(fact, name):
    f = fact(solves=0)
    rows = f.info("vtable_rows")
    assert rows > 0
    f.set_option(name, OWN_ACTION[name])
    assert f.info("vtable_rows") == rows
    f.set_option(name, 1 - OWN_ACTION[name])
    assert f.info("vtable_rows") == 0


@gpu
def test_plan_cache_trims_the_parked_plans(fact):
    f = fact(solves=0, superset_vtable=0)
    f.set_matrix(_problem(2, 40, 14)[0])
    f.set_matrix(_problem(3, 44, 16)[0])
    assert f.info("plans_cached") == 2
    f.set_option("plan_cache", 1)
    assert f.info("plans_cached") == 1
    f.set_option("plan_cache", -5)
    assert f.info("plans_cached") == 0


@gpu
def test_profile_collects_and_resets(fact):
    f = fact(solves=0)

    def counts():
        return sum(f.info(f"prof_{c}_count") for c in PROF_CLASSES)

    f.set_option("profile", 1)
    f.set_matrix(MAT)
    f.solve(RHS)
    f.solution_raw(0, f.N)
    seen = counts()
    assert seen > 0
    f.set_option("profile", 0)  # collects what is outstanding, keeps the sums
    assert counts() == seen
    f.set_option("profile", -1)
    assert counts() == 0


@gpu
def test_errors(fact):
    f = fact(solves=0)
    with pytest.raises(HipfactError) as e:
        f.set_option("no_such_option", 1)
    assert e.value.code == -1 and str(e.value) == "HIPFACT_EINVAL: unknown option: no_such_option"
    with pytest.raises(HipfactError) as e:
        f.set_option("multi_slice_rows", 17)
    assert e.value.code == -1 and str(e.value) == "HIPFACT_EINVAL: multi_slice_rows: 0 or a multiple of 16 in [16, 4096]"
    f.set_option("multi_slice_rows", 32)
    assert f.info("multi_slice_rows") == 32


@gpu
@pytest.mark.parametrize("var, value, key, want", [
    ("HIPFACT_XCD_CLASSES", "99", "xcd_classes", 16),
    ("HIPFACT_XCD_CLASSES", "0", "xcd_classes", 1),
    ("HIPFACT_GRAPH", "0", "use_graph", 0),
    ("HIPFACT_REFINE", "0", "refine_steps", 0),
    ("HIPFACT_REFINE", "3", "refine_steps", 3),
    ("HIPFACT_BOUNDARY_FAST", "0", "boundary_fast", 0),
    ("HIPFACT_XUPD_FUSED", "0", "xupd_fused", 0),
])
def test_environment_overrides_the_default_of_a_new_handle(monkeypatch, var, value, key, want):
    from sleqp_amd.fact import HipFact

    monkeypatch.setenv(var, value)
    f = HipFact(device=0)
    try:
        assert f.info(key) == want
    finally:
        f.free()


def test_every_option_of_the_header_has_a_class():
    text = open(os.path.join(ROOT, "include", "hipfact.h")).read()
    table = text[text.index("/* BEGIN OPTION TABLE"):text.index(" * END OPTION TABLE */")]
    names = re.findall(r'^ \*   "(\w+)"$', table, flags=re.M)
    assert len(names) == int(re.search(r"^ \* (\d+) options;", table, flags=re.M).group(1))
    classified = [n for c in CLASSES for n in c]
    assert sorted(classified) == sorted(names), set(classified) ^ set(names)
