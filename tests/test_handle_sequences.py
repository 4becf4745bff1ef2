"""The solve entry points interleaved on ONE handle, pair by pair (tests/handle_sequences.py has the nodes, the cases and
the walk).

Every other module tests its call on a fresh handle.  Here, per case, every node runs once alone behind the preamble
(the SOLO result, held to the truth by the bound of the module the call came with), and then one more handle runs a
closed walk in which every ordered pair of distinct nodes is adjacent exactly once: a few hundred calls, each compared
with its solo result bit for bit, with the state the contracts promise to leave alone checked behind each.  The
lifecycle test takes one handle through a refactorisation, smaller and larger working sets on the same superset plan,
another pattern and back, and lets two handles take turns on one device.

No number of its own: bit for bit, equality of codes and info blocks, or a bound imported by handle_sequences.

What the walk found is kept in FOUND (like test_fuzz_cases.FOUND): ordered pairs that once disagreed, run on a fresh
handle each."""
import time

import pytest

import handle_sequences as H

ESTATE = -5
# (case, first node, second node): what it found.  None of the three was a wrong result: the loops' projections stand
# in the check cadence of the single solve, which no header said; the rule is in include/hipfact.h now and
# handle_sequences.Walker pins it bit for bit against a handle that makes the counted calls alone
FOUND = [
    ("odd", "solve", "tr_lanczos", "a projection of the loop was checked here and not alone: num_checked, last_omega moved"),
    ("shifted", "solve", "tr_cg", "on a shifted factor every projection is checked and carries passes: num_passes moved"),
    ("sliced", "extra", "lsqr", "the same behind a call that is not remembered"),
]


def test_the_walk_has_every_ordered_pair_once():
    for n in (2, 3, len(H.NODES) - len(H.AUG_NODES), len(H.NODES)):
        w = H.closed_walk(n)
        assert len(w) == n * (n - 1) + 1 and H.walk_is_complete(w, n), n
    assert not H.walk_is_complete([0, 1, 0, 1, 0, 2, 0], 3)  # (a pair twice, others missing)
    assert [len(H.case(name).nodes) for name in ("assembled", "odd")] == [len(H.NODES), len(H.NODES) - len(H.AUG_NODES)]


_SOLO = {}


def _solo(c):
    """the solo results of a case, computed once for the tests that need them and left alone"""
    if c.name not in _SOLO:
        t = time.perf_counter()
        _SOLO[c.name] = H.solo_results(c)
        print("%s: %d solo handles in %.2f s" % (c.name, len(_SOLO[c.name]), time.perf_counter() - t))
    return _SOLO[c.name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", H.CASES)
def test_every_ordered_pair_on_one_handle(name):
    c = H.case(name)
    solo = _solo(c)
    assert not H.check_solo(c, solo)
    order = [c.nodes[i] for i in H.closed_walk(len(c.nodes))]
    s = H.Session(c)
    try:
        t = time.perf_counter()
        bad = H.run_walk(s, solo, order)  # (from its first vertex: the preamble's solve is another call than the node)
        print("%s: walk of %d calls in %.2f s" % (name, len(order), time.perf_counter() - t))
        assert not bad, "\n".join(bad)
        assert [s.f.info(k) for k in H.PLAN_KEYS] == s.plan_keys
        print("%s: multi_sliced_fronts %d, multi_single_cols %d" % (name, s.f.info("multi_sliced_fronts"), s.f.info("multi_single_cols")))
        for key in c.engaged:  # (the route the case is there for was taken)
            assert s.f.info(key) > 0, key
        s.f.check()  # (a refusal of the shifted factor has been reported by the call that met it, once)
    finally:
        s.free()


@pytest.mark.gpu
def test_found_pairs():
    bad = []
    for name, first, second in [f[:3] for f in FOUND]:
        c = H.case(name)
        s = H.Session(c)
        try:
            bad += H.run_walk(s, _solo(c), [first, second])
        finally:
            s.free()
    assert not bad, "\n".join(bad)


# ---- lifecycle ------------------------------------------------------------------------------------------------------------
def _fresh(c, nodes):
    """the nodes in order on a fresh handle brought to the case directly, behind the preamble"""
    s = H.Session(c)
    try:
        return [s.call(q) for q in nodes]
    finally:
        s.free()


def _compare(s, c, nodes, want):
    bad = []
    for q, w in zip(nodes, want):
        bad += ["%s, %s: %s" % (c.name, q, d) for d in H.same(s.call(q), w)]
    assert not bad, "\n".join(bad[:20])


def _refuses_the_old_border(s):
    """the border of an earlier factorisation is void: the state error, before any new hipfact_border_set"""
    assert s.f.info("border_k") == -1
    s.border = "a"  # (what the handle held; the right-hand side of that border)
    assert s.call("bordered_alone") == {"error": ESTATE}
    s.border = None


@pytest.mark.gpu
def test_lifecycle_of_one_handle():
    base, scaled, fewer, more, odd = H.case("assembled"), H.life_case("scaled"), H.life_case("fewer"), H.life_case("more"), H.case("odd")
    nodes = H.LIFE_NODES
    odd_nodes = ["solve", "multi_3", "border_a", "selinv", "gmres"]
    want = {c.name: _fresh(c, nodes) for c in (base, scaled, fewer, more)}
    want[odd.name] = _fresh(odd, odd_nodes)
    info = lambda k: s.f.info(k)  # noqa: E731
    s = H.Session(base)
    try:
        _compare(s, base, nodes, want[base.name])
        assert info("inactive_rows") == 2 and info("border_k") == base.border["a"].k and info("null_dim") == 0
        analyses, hits = info("analyses"), info("cache_hits")
        # 1. the same pattern with other values
        runs, calls = info("selinv_runs"), info("null_calls")
        s.load(scaled)
        assert info("analyses") == analyses and info("null_dim") == -1
        hits = info("cache_hits")
        _refuses_the_old_border(s)
        s.preamble()
        _compare(s, scaled, nodes, want[scaled.name])
        # (a regular K: hipfact_nullspace answers REGULAR without a pass, which "null_calls" does not count - the stamp
        # is what shows the recomputation here; test_a_refactorisation_recomputes_the_null_space has a shifted K)
        assert info("selinv_runs") == runs + 1 and info("null_dim") == 0 and info("null_calls") == calls
        # 2. three rows fewer, 3. more rows than at first: the same superset plan, N_ext shrinks and grows
        for c in (fewer, more):
            runs = info("selinv_runs")
            s.load(c)
            assert info("analyses") == analyses and info("cache_hits") == hits + 1
            hits += 1
            _refuses_the_old_border(s)
            s.preamble()
            _compare(s, c, nodes, want[c.name])
            assert info("selinv_runs") == runs + 1
        # 4. another pattern, then the first one again: the parked plan state comes back with every stamp void
        s.load(odd)
        assert info("analyses") == analyses + 1
        _refuses_the_old_border(s)
        s.preamble()
        _compare(s, odd, odd_nodes, want[odd.name])
        runs, hits = info("selinv_runs"), info("cache_hits")
        s.load(base)
        assert info("analyses") == analyses + 1 and info("cache_hits") == hits + 1
        assert info("null_dim") == -1
        _refuses_the_old_border(s)  # (d_bvec of this plan state still holds the Y of `more`)
        s.preamble()
        _compare(s, base, nodes, want[base.name])
        assert info("selinv_runs") == runs + 1
        s.f.check()
    finally:
        s.free()


@pytest.mark.gpu
def test_a_refactorisation_recomputes_the_null_space():
    """the counters of the lifecycle's first step where the null space takes passes: a shifted K, factored twice"""
    c = H.case("shifted")
    s = H.Session(c)
    try:
        one = s.call("nullspace")
        assert one["status"] == 1 and s.f.info("null_calls") == 1
        assert not H.same(s.call("nullspace"), one) and s.f.info("null_calls") == 1
        s.load(c)
        assert s.f.info("null_dim") == -1
        s.preamble()
        assert not H.same(s.call("nullspace"), one) and s.f.info("null_calls") == 2
    finally:
        s.free()


@pytest.mark.gpu
def test_two_handles_take_turns():
    """handle 1 makes a node of the walk of `odd`, handle 2 the next one, for 60 turns: both reproduce their solo bits"""
    c = H.case("odd")
    solo = _solo(c)
    order = [c.nodes[i] for i in H.closed_walk(len(c.nodes))]
    s1, s2 = H.Session(c), H.Session(c)
    walkers = []
    try:
        walkers.append(H.Walker(s1, solo))
        walkers.append(H.Walker(s2, solo))
        w1, w2 = walkers
        bad = []
        for i in range(100, 160):
            assert order[i] != order[i + 1]
            bad += ["handle 1: " + d for d in w1.step(order[i])]
            bad += ["handle 2: " + d for d in w2.step(order[i + 1])]
        assert not bad, "\n".join(bad[:20])
    finally:
        for w in walkers:
            w.close()
        s1.free()
        s2.free()
