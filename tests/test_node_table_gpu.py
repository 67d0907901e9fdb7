"""
The generic node table (LQRRT_MODEL_GENERIC: lqrrt_amd.engine.NodeTable, csrc/generic.hpp) at its size, width and tie edges,
against the NumPy model of tests/node_table_reference.py.

Acceptance of a query: the id is the model's, or the model's costs of the two ids differ by at most 1e-9 max(1, |cost|) (the last
bit of an atan2 may reorder two nodes) and the node is eligible; the returned cost is within the same bound of the model's cost of
the returned node.  Where no transcendental and no BLAS order is involved -- no angular state and S = identity, or caller-evaluated
error rows with S = identity -- id and cost are demanded EXACTLY: generic.hpp claims NumPy's summation order.

The interesting nodes are planted, not left to chance: a query equal to a node makes that node the unique winner (cost 0), two
identical nodes beyond the box of the random ones make an exact tie; every test asserts that the model's answer is the planted id.
"""
import ctypes as C
import time

import numpy as np
import pytest

from node_table_reference import NodeTableModel

pytestmark = pytest.mark.gpu

TOL = 1e-9
FAR = 9.0            # a coordinate outside the box [-6, 6] of the random nodes: where ties are planted


def _table(n, angles, capacity, **kw):
    from lqrrt_amd.engine import NodeTable
    return NodeTable(n, 2, angles, capacity=max(int(capacity), 2), **kw)       # (an engine holds at least two nodes)


def _dense(rs, n):
    A = rs.uniform(-1, 1, (n, n))
    return A.dot(A.T) + n * np.eye(n)


def _parents(rs, N):
    return np.concatenate(([-1], [rs.randint(0, i) for i in range(1, N)])).astype(np.int32)


def _lin(n, angles):
    """A non-angular state (ties are planted along it), or None."""
    free = [d for d in range(n) if d not in angles]
    return free[0] if free else None


def _set_flags(t, m, flags):
    """Replace the ignore set of table and model (one ABI call; NodeTable.ignore only adds)."""
    from lqrrt_amd import _native as nat
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    nat.check(nat.lib().lqrrt_tree_set_ignored(t.h, 0, len(flags), nat.ptr(flags)))
    m.ign = flags.astype(bool)


def _check(t, m, x, S=None, use_ignore=True, exact=False, expect=None, costs=None):
    """One host-form query against the model; returns what the table answered.  `costs`: the model's m.costs(x, S), where the
    caller computed it already."""
    if costs is None:
        costs = m.costs(x, S)
    want, cw = m.select(costs, use_ignore)
    if expect is not None:
        assert want == expect, "the model does not select the planted node: %d, planted %d" % (want, expect)
    got, c = t.nearest(x, S, use_ignore=use_ignore)
    assert 0 <= got < m.size
    if exact:
        assert (got, c) == (want, cw), (m.n, m.size, got, want, c, cw)
        return got, c
    if got != want:
        assert abs(costs[got] - cw) <= TOL * max(1.0, abs(cw)), (m.n, m.size, got, want, costs[got], cw)
        if use_ignore and not np.all(m.ign):
            assert not m.ign[got], "an ignored node was selected"
    assert abs(c - costs[got]) <= TOL * max(1.0, abs(costs[got])), (m.n, m.size, got, c, costs[got])
    return got, c


def _check_errors(t, m, x, use_ignore=True, expect=None):
    """The caller-evaluated form with S = identity: the rows are the model's, nothing transcendental on the device -> exact."""
    e = m.errors(x)
    costs = m.costs_of_errors(e)
    want, cw = m.select(costs, use_ignore)
    if expect is not None:
        assert want == expect
    assert t.nearest_from_errors(e, None, use_ignore=use_ignore) == (want, cw)


def _build(n, angles, nodes, pid, ignored=None, **kw):
    t = _table(n, angles, len(nodes), **kw)
    m = NodeTableModel(n, angles)
    t.load(nodes, pid, ignored)
    m.load(nodes, pid, ignored)
    return t, m


# ------------------------------------------------------------------------------------------------ a. reduce paths

def _reduce_regions(nb):
    """Partial indices the reduce handles in wave 1, 2, 3, in its `k += 256` stride, and the last one -- those that exist."""
    want = dict(wave1=64, wave2=128 + 9, wave3=192 + 60, stride=256, last=nb - 1)
    return {k: v for k, v in want.items() if v < nb}


@pytest.mark.parametrize("n,angles,N,tile", [(2, (1,), 16385 + 7, 256), (2, (1,), 65536 + 300, 256),
                                             (12, (), 16385 + 7, 256), (12, (), 65536 + 300, 256),
                                             (13, (), 16384 + 70, 64)])
def test_reduce_paths(n, angles, N, tile):
    """More than 64 / more than 256 partials: the unique winner planted in the tile of every reduce wave, of the stride loop and in the
    last, partial tile; exact ties between partials of different reduce waves (the lower id wins, whichever wave holds it); the
    batched form with one winner per region, bit for bit the host form."""
    rs = np.random.RandomState(100 + n + N)
    nb = (N + tile - 1) // tile
    assert nb > (256 if N > 60000 or tile == 64 else 64)
    regions = _reduce_regions(nb)
    assert "wave1" in regions and "last" in regions and N % tile != 0
    ids = {k: min(p * tile + 5, N - 1) for k, p in regions.items()}
    nodes = rs.uniform(-6, 6, (N, n))
    lin = _lin(n, angles)
    # tie pairs: identical nodes, far from the others, in partials of different reduce waves (and the stride loop, wave 0)
    pairs = [(ids["wave1"] + 1, 2 * tile + 7), (3 * tile + 1, ids["last"] - 1)]
    if "wave3" in regions:
        pairs += [(ids["wave2"] + 2, ids["wave3"] + 2), (ids["wave3"] + 3, ids["stride"] + 3)]
    for a, b in pairs:
        nodes[a, lin] = FAR
        nodes[b] = nodes[a]
    t, m = _build(n, angles, nodes, _parents(rs, N))
    Sd = _dense(rs, n)
    for S in (None, Sd):
        exact = S is None and not angles
        for k, i in sorted(ids.items()):
            assert _check(t, m, nodes[i].copy(), S, exact=exact, expect=i)[0] == i
        for a, b in pairs:
            x = nodes[a].copy()
            x[lin] += 0.5
            assert _check(t, m, x, S, exact=exact, expect=min(a, b))[0] == min(a, b)
    if not angles:
        _check_errors(t, m, nodes[ids["last"]].copy(), expect=ids["last"])
    if n <= 12:
        five = sorted(set(ids.values()))[:5]
        for p in (1, 33, 50, 20):                                  # (65 partials have two regions only: fill up from wave 0)
            if len(five) < 5:
                five.append(p * tile + 11)
        xs = nodes[five].copy()
        assert len({i // tile for i in five}) == 5                 # five partials, five reduce workgroups: (w nb + k) 2
        for S in (None, Sd):
            got_ids, got_costs = t.nn_argmin(xs, S)
            assert list(got_ids) == five
            for x, i, c in zip(xs, got_ids, got_costs):
                assert (int(i), float(c)) == t.nearest(x, S)
    t.close()


# ------------------------------------------------------------------------------------------------ b. grid stride of the scans

@pytest.mark.parametrize("n,angles,N,tile", [(2, (1,), 1048576 + 700, 256), (13, (), 262144 + 100, 64)])
def test_scan_grid_stride(n, angles, N, tile):
    """The smallest tables at which a scan workgroup strides over a second tile: workgroup 0 then holds ids >= 4096 tiles next to its
    first tile, so a lower-numbered workgroup can hold the HIGHER id of a tie."""
    t0 = time.time()
    rs = np.random.RandomState(7 + n)
    stride = tile * 4096
    assert stride < N <= stride + 4 * tile
    lo, hi = 300, stride + 5
    nodes = rs.uniform(-6, 6, (N, n))
    lin = _lin(n, angles)
    nodes[lo, lin] = FAR
    nodes[hi] = nodes[lo]
    pid = np.zeros(N, dtype=np.int32)
    pid[0] = -1
    tie = nodes[lo].copy()
    tie[lin] += 0.5
    beyond = N - 3                                                # a winner in the strided part
    Sd = _dense(rs, n)
    exact = not angles
    model_costs = {}

    def ask(x, S, want, use_ignore=True):
        """The planted id is what the model selects AND what the table answers: with an angular state the costs of the two tied
        nodes still are bit-equal (identical states), so the tolerance of _check alone would accept either id."""
        key = (x.tobytes(), S is None)                            # (the nodes stay: a million model costs once per query and S)
        if key not in model_costs:
            model_costs[key] = m.costs(x, S)
        got, _ = _check(t, m, x, S, use_ignore, exact=exact and S is None, expect=want, costs=model_costs[key])
        assert got == want, (n, N, got, want)

    t, m = _build(n, angles, nodes, pid)
    assert t.size == N
    ask(nodes[beyond].copy(), None, beyond)
    ask(tie, None, lo)                                            # id 300 (workgroup 1 or 4) against id stride + 5 (workgroup 0)
    ask(tie, Sd, lo)

    ign = rs.rand(N) < 0.3
    ign[lo], ign[hi], ign[beyond] = True, False, False
    t.load(nodes, pid, ign)
    m.load(nodes, pid, ign)
    ask(tie, None, hi)                                            # the lower id ignored: the strided one wins
    ask(tie, Sd, hi)
    ask(tie, None, lo, use_ignore=False)
    ask(tie, Sd, lo, use_ignore=False)
    ask(nodes[beyond].copy(), Sd, beyond)
    _check(t, m, rs.uniform(-6, 6, n), None, exact=exact)

    ign = np.ones(N, dtype=bool)
    t.load(nodes, pid, ign)
    m.load(nodes, pid, ign)
    assert np.all(t.ignored())
    ask(tie, None, lo)                                            # every node ignored: the overall nearest
    ask(tie, Sd, lo)
    ask(nodes[beyond].copy(), None, beyond)
    t.close()
    print("test_scan_grid_stride n=%d N=%d: %.2f s" % (n, N, time.time() - t0))


# ------------------------------------------------------------------------------------------------ c. small sizes and word edges

SMALL_N = (1, 2, 63, 64, 65, 255, 256, 257)


def _small_case(t, m, nodes, rs, reload):
    """Queries of one small table under the four ignore sets; `reload`: apply a set by load(..., ignored=) instead of the flag call."""
    n, N, angles = m.n, m.size, m.angle_dims
    Sd = _dense(rs, n)
    xr = rs.uniform(-6, 6, n)
    queries = [xr, nodes[N - 1].copy(), nodes[N // 2] + 1e-3]
    sets = [("none", np.zeros(N, dtype=bool), [])]
    but_last = np.ones(N, dtype=bool)
    but_last[N - 1] = False
    sets.append(("all but the last", but_last, []))
    nearest = np.zeros(N, dtype=bool)
    nearest[m.select(m.costs(xr), use_ignore=False)[0]] = True
    sets.append(("the overall nearest", nearest, []))
    if N >= 65:
        word0 = np.zeros(N, dtype=bool)
        word0[:64] = True
        sets.append(("ids 0..63", word0, [(nodes[64].copy(), 64)]))
    for name, flags, planted in sets:
        if reload:
            t.load(m.state.copy(), m.pID.copy(), flags)
            m.load(m.state.copy(), m.pID.copy(), flags)
        else:
            _set_flags(t, m, flags)
        np.testing.assert_array_equal(t.ignored(), flags)
        for S in (None, Sd):
            exact = S is None and not angles
            for use_ignore in (True, False):
                for x in queries:
                    _check(t, m, x, S, use_ignore, exact=exact)
                for x, i in planted:
                    _check(t, m, x, S, use_ignore, exact=exact, expect=i)
        if name == "all but the last":
            assert t.nearest(xr, None, use_ignore=True)[0] == N - 1       # the only eligible node sits in the last, partial tile
        _check_errors(t, m, xr, use_ignore=True)
        if n <= 12:                                               # max_wave = 1: the batched form takes exactly one query
            i1, c1 = t.nn_argmin(xr[None, :], None)
            assert (int(i1[0]), float(c1[0])) == t.nearest(xr, None)
            i1, c1 = t.nn_argmin(xr[None, :], Sd, use_ignore=False)
            assert (int(i1[0]), float(c1[0])) == t.nearest(xr, Sd, use_ignore=False)
    if n <= 12:
        from lqrrt_amd import _native as nat
        with pytest.raises(nat.NativeError, match="exceeds max_wave=1") as refused:     # the engine's refusal, not a wrapper's error
            t.nn_argmin(np.vstack((xr, xr)), None)
        assert refused.value.code == nat.E_CAPACITY


@pytest.mark.parametrize("n,angles", [(1, ()), (1, (0,)), (7, ()), (7, (0, 6)), (8, (2,)), (12, ()), (12, (3, 11)),
                                      (13, ()), (13, (0, 12)), (16, (5,)), (64, ()), (64, (1, 63))])
def test_small_sizes_and_word_edges(n, angles):
    """capacity == N, max_wave = 1, N at the edges of the 64-bit ignore words and of the 64- and 256-node tiles; built by load and by
    reset + append; states() / parents() exactly the model's."""
    rs = np.random.RandomState(1000 + 17 * n + len(angles))
    for N in SMALL_N:
        nodes = rs.uniform(-6, 6, (N, n))
        pid = _parents(rs, N)
        for by_append in (False, True):
            t = _table(n, angles, N, max_wave=1)
            m = NodeTableModel(n, angles)
            if by_append:
                t.reset(nodes[0])
                m.reset(nodes[0])
                for i in range(1, N):
                    t.append(int(pid[i]), nodes[i])
                    m.append(int(pid[i]), nodes[i])
            else:
                t.load(nodes, pid)
                m.load(nodes, pid)
            assert t.size == m.size == N
            np.testing.assert_array_equal(t.states(), m.state)
            np.testing.assert_array_equal(t.parents(), m.pID)
            np.testing.assert_array_equal(t.ignored(), m.ignored())
            _small_case(t, m, nodes, rs, reload=not by_append)
            np.testing.assert_array_equal(t.states(), m.state)
            t.close()


# ------------------------------------------------------------------------------------------------ d. full tables, max_wave 1..3

@pytest.mark.parametrize("max_wave", [1, 2, 3])
@pytest.mark.parametrize("n,angles", [(16, (1, 15)), (5, (2,))])
def test_full_table_small_max_wave(n, angles, max_wave):
    """capacity = N = 1024 with max_wave 1, 2, 3: a full wide table writes 16 partial pairs, more than the 4 max_wave pairs its
    buffers held before they were sized from generic_sizes.hpp."""
    rs = np.random.RandomState(31 * n + max_wave)
    N = 1024
    nodes = rs.uniform(-6, 6, (N, n))
    t, m = _build(n, angles, nodes, _parents(rs, N), max_wave=max_wave)
    ign = rs.rand(N) < 0.3
    _set_flags(t, m, ign)
    Sd = _dense(rs, n)
    planted = [0, 63, 64, 255, 256, 511, 767, 960, 1023]
    for S in (None, Sd):
        for use_ignore in (True, False):
            for x in rs.uniform(-6, 6, (16, n)):
                _check(t, m, x, S, use_ignore)
            for i in planted:
                _check(t, m, nodes[i].copy(), S, use_ignore, expect=None if (use_ignore and ign[i]) else i)
    _check_errors(t, m, nodes[1023].copy(), use_ignore=False, expect=1023)
    t.close()


# ------------------------------------------------------------------------------------------------ e. many angular states

def _angles_64():
    return tuple(sorted(set(range(0, 64, 2)) | set(range(49, 64, 2))))        # every second index, then the top ones: 40 of 64


SPECIAL = [0.0, np.pi, -np.pi, np.pi - 1e-12, -np.pi + 1e-12, 100.0, -100.0, 0.5, 0.5 + np.pi, -2.0, -2.0 + np.pi]


@pytest.mark.parametrize("n,angles", [(12, tuple(range(12))), (16, tuple(range(16))), (64, _angles_64())])
def test_many_angular_states(n, angles):
    """More angular states than GenericShape::wd holds on the wide path, all of them on the narrow one; angles at 0, +-pi, next to
    +-pi, many turns away, and pairs exactly pi apart.  Costs are compared (an error of +pi or -pi costs the same)."""
    assert len(angles) == (40 if n == 64 else n)
    rs = np.random.RandomState(55 + n)
    N = 300
    nodes = rs.uniform(-6, 6, (N, n))
    for i in range(0, N, 3):                                      # a third of the nodes: special values in some angular columns
        for d in rs.choice(angles, 4, replace=False):
            nodes[i, d] = SPECIAL[rs.randint(len(SPECIAL))]
    nodes[7, list(angles)] = np.pi
    nodes[8, list(angles)] = -np.pi
    nodes[9, list(angles)] = 0.0
    t, m = _build(n, angles, nodes, _parents(rs, N))
    np.testing.assert_array_equal(t.states(), nodes)
    Sd = _dense(rs, n)
    queries = [rs.uniform(-6, 6, n) for _ in range(6)]
    for v in SPECIAL:
        x = rs.uniform(-6, 6, n)
        x[list(angles)] = v
        queries.append(x)
    queries += [nodes[7].copy(), nodes[8].copy(), nodes[150].copy()]
    ign = rs.rand(N) < 0.3
    _set_flags(t, m, ign)
    for S in (None, Sd):
        for use_ignore in (True, False):
            for x in queries:
                _check(t, m, x, S, use_ignore)
    t.close()


@pytest.mark.parametrize("n,bad", [(4, (2, 1)), (4, (1, 1)), (4, (4,)), (4, (-1,)), (16, (0, 15, 3)), (16, (16,)), (64, (5, 5))])
def test_bad_angle_dims_are_refused(n, bad):
    """Unsorted, duplicate or out-of-range angular indices: an exception from NodeTable, and an error code from the C ABI before
    anything is allocated or launched (no engine comes back)."""
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import NodeTable
    with pytest.raises(ValueError):
        NodeTable(n, 1, bad, capacity=128)
    d = nat.SystemDesc()
    d.model, d.nstates, d.ncontrols = nat.MODEL_GENERIC, n, 1
    d.n_params = 1 + len(bad)
    d.params[0] = float(len(bad))
    for k, dim in enumerate(bad):
        d.params[1 + k] = float(dim)
    h = C.c_void_p()
    assert nat.lib().lqrrt_engine_create(C.byref(d), 0, 128, 1, C.byref(h)) == nat.E_ARG
    assert not h.value


# ------------------------------------------------------------------------------------------------ f. stale ignore bits

@pytest.mark.parametrize("n,angles", [(4, (2,)), (14, (3,))])
def test_no_stale_ignore_bits(n, angles):
    """Ignore bits of nodes that went away (truncate, load, reset) must not come back for the nodes appended over their ids."""
    rs = np.random.RandomState(77 + n)
    t = _table(n, angles, 512)
    m = NodeTableModel(n, angles)

    def verify(own=()):
        np.testing.assert_array_equal(t.ignored(), m.ignored())
        assert t.size == m.size
        for x in rs.uniform(-6, 6, (5, n)):
            _check(t, m, x, None, use_ignore=True)
        for i in own:                                             # a node is the nearest to itself unless it is ignored
            _check(t, m, m.state[i].copy(), None, use_ignore=True, expect=None if m.ign[i] else i)

    def grow(upto):
        while m.size < upto:
            x, p = rs.uniform(-6, 6, n), int(rs.randint(0, m.size))
            t.append(p, x)
            m.append(p, x)

    nodes = rs.uniform(-6, 6, (400, n))
    pid = _parents(rs, 400)
    t.load(nodes, pid)
    m.load(nodes, pid)
    t.ignore(range(100, 200))
    m.ignore(range(100, 200))
    verify(own=(99, 100, 150, 199, 200))
    t.truncate(50)
    m.truncate(50)
    verify(own=(0, 49))
    for k in range(20):                                           # append and ask at once ...
        grow(m.size + 1)
        _check(t, m, m.state[-1].copy(), None, use_ignore=True, expect=m.size - 1)
    grow(250)                                                     # ... and in bulk: ids 50..249 cover the old flags 100..199
    assert not m.ign.any()
    verify(own=range(50, 250))
    t.ignore([60])
    m.ignore([60])
    verify(own=(59, 60, 61, 128))
    nodes2 = rs.uniform(-6, 6, (70, n))
    pid2 = _parents(rs, 70)
    t.load(nodes2, pid2)
    m.load(nodes2, pid2)
    verify(own=(59, 60, 61, 69))
    grow(131)
    verify(own=range(60, 131))
    x0 = rs.uniform(-6, 6, n)
    t.reset(x0)
    m.reset(x0)
    grow(11)
    verify(own=range(11))
    np.testing.assert_array_equal(t.states(), m.state)
    np.testing.assert_array_equal(t.parents(), m.pID)
    t.close()


# ------------------------------------------------------------------------------------------------ g. side stream

def test_side_stream():
    """The mid-size case n = 6 with angles, N = 257, built by load and by append, with a side stream current: the copies of a bulk
    load are queued on the stream of the kernel that derives the trig rows from them.  (Before, they went through blocking copies
    on the null stream and only the kernel on the side stream; that order usually held anyway, so this test cannot be made to fail
    deterministically on the old code -- it guards the explicit ordering.)  The same holds for states() / parents() right after the
    appends: torch's side streams are non-blocking, so the read-back (blocking copies on the null stream) waits for the device."""
    import torch
    n, angles, N = 6, (2, 5), 257
    rs = np.random.RandomState(9)
    nodes = rs.uniform(-6, 6, (N, n))
    pid = _parents(rs, N)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for by_append in (False, True):
            t = _table(n, angles, N, max_wave=1)
            m = NodeTableModel(n, angles)
            assert t._stream.value == side.cuda_stream
            if by_append:
                t.reset(nodes[0])
                m.reset(nodes[0])
                for i in range(1, N):
                    t.append(int(pid[i]), nodes[i])
                    m.append(int(pid[i]), nodes[i])
            else:
                t.load(nodes, pid)
                m.load(nodes, pid)
            np.testing.assert_array_equal(t.states(), m.state)
            np.testing.assert_array_equal(t.parents(), m.pID)
            _small_case(t, m, nodes, rs, reload=not by_append)
            t.close()
    side.synchronize()
