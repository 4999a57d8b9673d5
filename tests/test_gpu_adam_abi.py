"""gae_adam_step / gae_x_adam_step_tail (K12, csrc/optim.hip) through the raw C ABI against tests/adam_ref.py: the
order in which deferred partial-sum lists are added (bit for bit, at every list length and block tail where the code
changes form, in three layouts), the tensor lookup of a mixed 16-tensor launch, the update rule against float64 at the
hyper-parameter edges, the six words of device state, the argument errors, and the stand-alone reduction launch of
the weight-gradient kernels tied to the same reference.

Every param / grad / exp_avg / exp_avg_sq buffer sits between two guards of 64 floats that hold a NaN bit pattern, and
every float around a partial-sum list is NaN: a write outside [0, n) changes a guard, a read outside poisons a sum."""
import ctypes
import fractions

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = R.GUARD
PATTERN = 0x7FC0BEEF                 # a quiet NaN
PARAM, GRAD, EXP_AVG, EXP_AVG_SQ = range(4)
ENTRIES = ["gae_adam_step", "gae_x_adam_step_tail"]        # the second one with tail = NULL: the same launch
DEFAULTS = (1e-2, 0.9, 0.999, 1e-8)                         # lr, beta1, beta2, eps
E_NULL, E_SIZE, E_RANGE = -1, -2, -6
# beta^t after the pow path (fresh / resumed counter, changed betas): one double pow, taken at <= 2 ulp, and one
# rounded multiplication by beta: (2 + 1/2) 2^-52 relative
POW_PATH = 3 * 2.0 ** -52


class Arena:
    """param, grad, exp_avg, exp_avg_sq of the tensors of one launch in ONE device buffer, each between two guards.
    An empty tensor owns one dummy float per buffer (never NULL in a launch); it counts as guard."""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        self.off, pos = [], 0
        for n in self.sizes:
            w = max(n, 1) + 2 * GUARD
            self.off.append([pos + j * w + GUARD for j in range(4)])
            pos += 4 * w
        self.host = np.full(pos, PATTERN, np.uint32)
        self.inside = np.zeros(pos, bool)
        for n, o in zip(self.sizes, self.off):
            for j in range(4):
                self.inside[o[j]:o[j] + n] = True
        self.dev = torch.empty(pos, dtype=torch.int32, device=DEV)

    def ptr(self, k, j):
        return self.dev.data_ptr() + 4 * self.off[k][j]

    def set(self, k, j, values):
        o, n = self.off[k][j], self.sizes[k]
        self.host[o:o + n] = np.ascontiguousarray(values, np.float32).reshape(n).view(np.uint32)

    def poison(self, k, j):
        o, n = self.off[k][j], self.sizes[k]
        self.host[o:o + n] = PATTERN

    def bits(self, k, j):
        o, n = self.off[k][j], self.sizes[k]
        return self.host[o:o + n].copy()

    def get(self, k, j):
        return self.bits(k, j).view(np.float32)

    def upload(self):
        self.dev.copy_(torch.from_numpy(self.host.view(np.int32)))

    def download(self):
        torch.cuda.synchronize()
        self.host = self.dev.cpu().numpy().view(np.uint32).copy()

    def guards_intact(self):
        return bool(np.all(self.host[~self.inside] == PATTERN))


class Lists:
    """the partial-sum lists of one launch in one device buffer (adam_ref.place_partials: NaN wherever no element is)"""

    def __init__(self):
        self.bufs, self.offs, self.pos, self.dev = [], [], 0, None

    def add(self, P, stride, row_len, row_pitch):
        buf = R.place_partials(P, stride, row_len, row_pitch)
        self.offs.append(self.pos + GUARD)
        self.bufs.append(buf)
        self.pos += buf.size
        return len(self.offs) - 1

    def upload(self):
        self.host = np.concatenate(self.bufs) if self.bufs else np.full(2 * GUARD, np.nan, np.float32)
        self.dev = torch.from_numpy(self.host).to(DEV)

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.offs[i]

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host.view(np.uint32))


def descriptor(arena, k, lists=None, li=None, n_partials=0, lay=(0, 1, 1), n=None):
    from gae_dgl_amd import _lib
    return _lib.AdamTensor(arena.ptr(k, PARAM), arena.ptr(k, GRAD), arena.ptr(k, EXP_AVG), arena.ptr(k, EXP_AVG_SQ),
                           arena.sizes[k] if n is None else n, lists.ptr(li) if n_partials else None, n_partials,
                           lay[0], lay[1], lay[2])


def launch(descs, hyper, state, entry="gae_adam_step", n_tensors=None, raw=False):
    """one call of the entry point as optim.Adam.step makes it; raw=True returns the status instead of raising"""
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _stream
    arr = (_lib.AdamTensor * max(len(descs), 1))(*descs)
    args = [arr, len(descs) if n_tensors is None else n_tensors] + [float(x) for x in hyper]
    args.append(ctypes.c_void_p(state.data_ptr()) if state is not None else None)
    if entry == "gae_x_adam_step_tail":
        args.append(None)
    with torch.cuda.device(DEV):
        args.append(_stream())
        if raw:
            return int(getattr(_lib.load(), entry)(*args))
        _lib.call(entry, *args)
    return 0


def new_state(words=(0, 0, 0, 0, 0, 0)):
    return torch.tensor(list(words), dtype=torch.int64, device=DEV)


def read_state(state):
    """(the six words, the same bytes as doubles)"""
    w = state.cpu().numpy().copy()
    return w, w.view(np.float64)


def double_bits(x):
    return int(np.array([x], np.float64).view(np.int64)[0])


def power_error(cached, beta, t):
    """relative error of a cached double against beta^t in exact rational arithmetic"""
    exact = fractions.Fraction(beta) ** t
    return float(abs(fractions.Fraction(float(cached)) - exact) / exact) if exact else abs(float(cached))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 1. order and layout
@pytest.mark.parametrize("kind", R.LAYOUTS)
def test_deferred_sum_has_the_library_order_in_every_form(kind):
    """lr = 0: the launch only adds the list and updates the moments.  Written gradient == adam_ref.sum_in_library_order
    bit for bit and within the rounding bound of the float64 sum, param untouched, moments against float64, counter 1"""
    hyper = (0.0,) + DEFAULTS[1:] + (0.0,)
    h = tuple(R.f32(x) for x in hyper)
    rng = np.random.default_rng(11)
    worst = {"sum / bound": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    launches = 0
    for q in R.LIST_LENGTHS:
        for n in R.sizes_for(q):
            what = f"{kind}: {q} partials of {n} elements"
            P = R.wide_partials(q, n)
            lay = R.layout(kind, n)
            arena = Arena([n])
            p0 = rng.standard_normal(n).astype(np.float32)
            m0 = rng.standard_normal(n).astype(np.float32)
            v0 = rng.random(n).astype(np.float32)
            arena.set(0, PARAM, p0); arena.set(0, EXP_AVG, m0); arena.set(0, EXP_AVG_SQ, v0)    # grad: the NaN pattern
            lists = Lists()
            li = lists.add(P, *lay)
            arena.upload(); lists.upload()
            state = new_state()
            launch([descriptor(arena, 0, lists, li, q, lay)], hyper, state, ENTRIES[launches % 2])
            launches += 1
            arena.download()
            assert arena.guards_intact(), what
            g = arena.get(0, GRAD)
            want = R.sum_in_library_order(P)
            assert not np.isnan(g).any(), what
            assert same_bits(g, want), (what, int((g.view(np.uint32) != want.view(np.uint32)).sum()))
            ratio = float((np.abs(g.astype(np.float64) - P.astype(np.float64).sum(0)) / R.sum_bound(P)).max())
            worst["sum / bound"] = max(worst["sum / bound"], ratio)
            assert ratio <= 1.0, (what, ratio)
            assert same_bits(arena.get(0, PARAM), p0), what
            _, m_ref, v_ref = R.adam_fp64(p0, g, m0, v0, 1, *h)
            em, ev = R.rel_err(arena.get(0, EXP_AVG), m_ref), R.rel_err(arena.get(0, EXP_AVG_SQ), v_ref)
            worst["exp_avg"] = max(worst["exp_avg"], em); worst["exp_avg_sq"] = max(worst["exp_avg_sq"], ev)
            assert em < R.TRAJECTORY_BOUND and ev < R.TRAJECTORY_BOUND, (what, em, ev)
            w, _ = read_state(state)
            assert w[0] == 1 and w[1] == 0, (what, w)
    print(f"order and layout, {kind}: {launches} launches, largest " +
          ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (bounds 1, {R.TRAJECTORY_BOUND:g}, {R.TRAJECTORY_BOUND:g})")


# ---------------------------------------------------------------------------------------------- 2. / 3. trajectories
def run_trajectory(spec, steps, hyper, entry="gae_adam_step", seed=0):
    """`steps` launches over the tensors spec = [(n, n_partials)]: gradients and partials redrawn per step as
    N(0, 1) (1 + it), the deferred tensors' lists in the three layouts in turn.  Per step: guards, counter, ticket,
    written gradients == the library order.  Returns the largest rel_err of param / exp_avg / exp_avg_sq against
    adam_fp64 stepping on the gradients as written back, after the last step and over all steps."""
    h = tuple(R.f32(x) for x in hyper)
    arena = Arena([n for n, _ in spec])
    rng = np.random.default_rng(seed)
    ref = []
    for k, (n, _) in enumerate(spec):
        p0 = rng.standard_normal(n).astype(np.float32)
        arena.set(k, PARAM, p0); arena.set(k, EXP_AVG, np.zeros(n)); arena.set(k, EXP_AVG_SQ, np.zeros(n))
        ref.append((p0.astype(np.float64), np.zeros(n), np.zeros(n)))
    state = new_state()
    last, over_steps = [0.0] * 3, [0.0] * 3
    for it in range(steps):
        lists, deferred, want = Lists(), {}, []
        for k, (n, q) in enumerate(spec):
            if q == 0:
                g = (rng.standard_normal(n) * (1.0 + it)).astype(np.float32)
                arena.set(k, GRAD, g)
                want.append(g)
            else:
                P = (rng.standard_normal((q, n)) * (1.0 + it)).astype(np.float32)
                lay = R.layout(R.LAYOUTS[len(deferred) % 3], n)
                deferred[k] = (lists.add(P, *lay), q, lay)
                arena.poison(k, GRAD)
                want.append(R.sum_in_library_order(P))
        arena.upload(); lists.upload()
        descs = [descriptor(arena, k, lists, *deferred[k]) if k in deferred else descriptor(arena, k)
                 for k in range(len(spec))]
        launch(descs, hyper, state, entry)
        arena.download()
        w, _ = read_state(state)
        assert w[0] == it + 1 and w[1] == 0, (it, w)
        assert arena.guards_intact(), it
        last = [0.0] * 3
        for k, (n, q) in enumerate(spec):
            g = arena.get(k, GRAD)
            assert same_bits(g, want[k]), (it, k, spec[k])
            ref[k] = R.adam_fp64(ref[k][0], g, ref[k][1], ref[k][2], it + 1, *h)
            for j, buf in enumerate((PARAM, EXP_AVG, EXP_AVG_SQ)):
                got = arena.get(k, buf)
                assert np.isfinite(got).all(), (it, k, spec[k])
                last[j] = max(last[j], R.rel_err(got, ref[k][j]))
        over_steps = [max(a, b) for a, b in zip(over_steps, last)]
    return last, over_steps


@pytest.mark.parametrize("wd", R.WEIGHT_DECAYS)
@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_mixed_launch_trajectory_against_fp64(order, wd):
    """16 tensors of every kind in one launch (three block sizes, empty tensors, every tail), 25 steps"""
    spec = R.MIXED if order == "listed" else R.MIXED[::-1]
    last, over = run_trajectory(spec, 25, DEFAULTS + (wd,), ENTRIES[order == "reversed"], seed=2)
    print(f"mixed launch, {order}, weight_decay {wd:g}: rel_err after 25 steps param {last[0]:.3g}, exp_avg "
          f"{last[1]:.3g}, exp_avg_sq {last[2]:.3g}; largest over the steps {max(over):.3g} (bound {R.TRAJECTORY_BOUND:g})")
    assert max(last) < R.TRAJECTORY_BOUND, last


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_launch_of_empty_tensors_writes_nothing_and_counts_one_step(entry):
    """every tensor empty, the last one with a partial list (dummy buffers, never NULL): one block runs, nothing is
    written, the counter still advances"""
    arena = Arena([n for n, _ in R.ALL_EMPTY])
    lists, deferred = Lists(), {}
    for k, (n, q) in enumerate(R.ALL_EMPTY):
        if q:
            lay = R.layout("padded_rows", n)
            deferred[k] = (lists.add(np.zeros((q, 0), np.float32), *lay), q, lay)
    arena.upload(); lists.upload()
    state = new_state()
    descs = [descriptor(arena, k, lists, *deferred[k]) if k in deferred else descriptor(arena, k)
             for k in range(len(R.ALL_EMPTY))]
    for step in (1, 2):
        launch(descs, DEFAULTS + (0.0,), state, entry)
        arena.download()
        assert arena.guards_intact() and lists.unchanged()
        w, d = read_state(state)
        assert w[0] == step and w[1] == 0
        assert w[2] == double_bits(R.f32(0.9)) and w[4] == double_bits(R.f32(0.999))


@pytest.mark.parametrize("wd", R.WEIGHT_DECAYS)
@pytest.mark.parametrize("betas", R.EDGE_BETAS)
def test_hyper_parameter_edges(betas, wd):
    """5 steps on one plain tensor and one 33-partial tensor (5, not 25: at betas (0, 0) an fp32 restatement of the
    rule is itself 5.4e-6 from float64 after 25 steps, 7.8e-7 after 5)"""
    last, _ = run_trajectory([(257, 0), (257, 33)], 5, (DEFAULTS[0],) + betas + (DEFAULTS[3], wd), seed=3)
    print(f"betas {betas}, weight_decay {wd:g}: rel_err after 5 steps param {last[0]:.3g}, exp_avg {last[1]:.3g}, "
          f"exp_avg_sq {last[2]:.3g} (bound {R.TRAJECTORY_BOUND:g})")
    assert max(last) < R.TRAJECTORY_BOUND, last


def test_zero_learning_rate():
    last, _ = run_trajectory([(257, 0), (257, 33)], 5, (0.0,) + DEFAULTS[1:] + (0.0,), seed=4)
    print(f"lr 0: rel_err after 5 steps param {last[0]:.3g}, exp_avg {last[1]:.3g}, exp_avg_sq {last[2]:.3g}")
    assert last[0] == 0.0 and max(last) < R.TRAJECTORY_BOUND, last


# ---------------------------------------------------------------------------------------------- 4. step state
def _small(n=4, seed=6):
    rng = np.random.default_rng(seed)
    arena = Arena([n])
    vals = [rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.random(n).astype(np.float32) + 0.5]
    for j, x in enumerate(vals):
        arena.set(0, j, x)
    arena.upload()
    return arena, vals


def test_state_words_of_a_fresh_counter():
    """[k, 0, bits(double(beta1)), beta1^k, bits(double(beta2)), beta2^k]: one rounding per cached multiplication"""
    arena, _ = _small()
    b1, b2 = R.f32(DEFAULTS[1]), R.f32(DEFAULTS[2])
    state = new_state()
    for k in range(1, 6):
        launch([descriptor(arena, 0)], DEFAULTS + (0.0,), state)
        w, d = read_state(state)
        assert w[0] == k and w[1] == 0, w
        assert w[2] == double_bits(b1) and w[4] == double_bits(b2), w
        e1, e2 = power_error(d[3], b1, k), power_error(d[5], b2, k)
        assert e1 <= k * 2.0 ** -52 and e2 <= k * 2.0 ** -52, (k, e1, e2)
    arena.download()
    assert arena.guards_intact()


def test_cached_powers_after_2000_launches():
    arena, _ = _small()
    b1, b2 = R.f32(DEFAULTS[1]), R.f32(DEFAULTS[2])
    state = new_state()
    desc = [descriptor(arena, 0)]
    for _ in range(2000):
        launch(desc, DEFAULTS + (0.0,), state)
    w, d = read_state(state)
    e1, e2 = power_error(d[3], b1, 2000), power_error(d[5], b2, 2000)
    print(f"2000 launches: beta1^t off by {e1:.3g}, beta2^t by {e2:.3g} relative (bound {2000 * 2.0 ** -52:.3g})")
    assert w[0] == 2000 and w[1] == 0
    assert w[2] == double_bits(b1) and w[4] == double_bits(b2)
    assert e1 <= 2000 * 2.0 ** -52 and e2 <= 2000 * 2.0 ** -52
    arena.download()
    assert arena.guards_intact() and np.isfinite(arena.get(0, PARAM)).all()


def test_resume_from_a_preset_counter():
    """state [1000, 0, 0, 0, 0, 0] and preset moments: the step is step 1001, and the cache is left valid for it"""
    arena, (p0, g0, m0, v0) = _small(n=257)
    h = tuple(R.f32(x) for x in DEFAULTS + (0.0,))
    state = new_state((1000, 0, 0, 0, 0, 0))
    launch([descriptor(arena, 0)], DEFAULTS + (0.0,), state)
    arena.download()
    assert arena.guards_intact() and same_bits(arena.get(0, GRAD), g0)
    ref = R.adam_fp64(p0, g0, m0, v0, 1001, *h)
    errs = [R.rel_err(arena.get(0, j), r) for j, r in zip((PARAM, EXP_AVG, EXP_AVG_SQ), ref)]
    print(f"resume at 1000: rel_err {errs} (bound {R.TRAJECTORY_BOUND:g})")
    assert max(errs) < R.TRAJECTORY_BOUND, errs
    not_resumed = R.adam_fp64(p0, g0, m0, v0, 1, *h)[0]
    assert R.rel_err(ref[0], not_resumed) > 100 * R.TRAJECTORY_BOUND          # the comparison sees the step count
    w, d = read_state(state)
    assert w[0] == 1001 and w[1] == 0 and w[2] == double_bits(h[1]) and w[4] == double_bits(h[2])
    assert power_error(d[3], h[1], 1001) <= POW_PATH and power_error(d[5], h[2], 1001) <= POW_PATH


def test_changed_betas_take_the_pow_path_then_the_cache():
    """3 steps at (0.9, 0.999), then 2 at (0.8, 0.99): torch's rule -- the current betas' powers at the running count"""
    arena, (p0, _, _, _) = _small(n=257)
    n = 257
    arena.set(0, EXP_AVG, np.zeros(n)); arena.set(0, EXP_AVG_SQ, np.zeros(n))
    rng = np.random.default_rng(8)
    ref = (p0.astype(np.float64), np.zeros(n), np.zeros(n))
    state = new_state()
    words = []
    for it in range(5):
        betas = (0.9, 0.999) if it < 3 else (0.8, 0.99)
        hyper = (DEFAULTS[0],) + betas + (DEFAULTS[3], 0.0)
        h = tuple(R.f32(x) for x in hyper)
        g = (rng.standard_normal(n) * (1.0 + it)).astype(np.float32)
        arena.set(0, GRAD, g)
        arena.upload()
        launch([descriptor(arena, 0)], hyper, state)
        arena.download()
        assert arena.guards_intact()
        ref = R.adam_fp64(ref[0], g, ref[1], ref[2], it + 1, *h)
        errs = [R.rel_err(arena.get(0, j), r) for j, r in zip((PARAM, EXP_AVG, EXP_AVG_SQ), ref)]
        assert max(errs) < R.TRAJECTORY_BOUND, (it, errs)
        w, d = read_state(state)
        assert w[0] == it + 1 and w[1] == 0 and w[2] == double_bits(h[1]) and w[4] == double_bits(h[2]), (it, w)
        words.append((d[3], d[5], h[1], h[2]))
    # step 4 (the switch): pow(beta, 3) beta of the NEW betas -- the cache would have given 0.9^3 0.8
    assert power_error(words[3][0], words[3][2], 4) <= POW_PATH and power_error(words[3][1], words[3][3], 4) <= POW_PATH
    # step 5: the cached power times beta, one double multiplication
    assert words[4][0] == words[3][0] * words[4][2] and words[4][1] == words[3][1] * words[4][3]
    # steps 2 and 3 came from the cache as well
    for it in (1, 2):
        assert words[it][0] == words[it - 1][0] * words[it][2] and words[it][1] == words[it - 1][1] * words[it][3]


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_return_before_any_launch(entry):
    from gae_dgl_amd import _lib
    arena, _ = _small(n=8)
    lists = Lists()
    li = lists.add(np.ones((3, 8), np.float32), 8, 8, 8)
    lists.upload()
    before = arena.host.copy()
    state = new_state((3, 0, 0, 0, 0, 0))
    ok = DEFAULTS + (0.0,)
    good = descriptor(arena, 0)
    cases = [
        ("17 tensors", [good] * 17, ok, state, E_RANGE),
        ("negative n", [descriptor(arena, 0, n=-1)], ok, state, E_SIZE),
        ("beta1 = 1", [good], (1e-2, 1.0, 0.999, 1e-8, 0.0), state, E_RANGE),
        ("lr < 0", [good], (-1e-2, 0.9, 0.999, 1e-8, 0.0), state, E_RANGE),
        ("row_len = 0", [descriptor(arena, 0, lists, li, 3, (8, 0, 8))], ok, state, E_SIZE),
        ("NULL state", [good], ok, None, E_NULL),
    ]
    for what, descs, hyper, st, code in cases:
        assert launch(descs, hyper, st, entry, raw=True) == code, what
        assert _lib.load().gae_last_error(), what
    # no tensors and no tail: OK, nothing launched, the counter stays
    assert launch([], ok, state, entry, raw=True) == 0
    arena.download()
    assert np.array_equal(arena.host, before) and lists.unchanged()
    w, _ = read_state(state)
    assert list(w) == [3, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- 5. the stand-alone reduction
def _raw_list(entry, n):
    """the list [n_partials, n] a deferred weight-gradient kernel left in its workspace, copied to the host"""
    ws, ptr, q, stride, row_len, row_pitch = entry
    flat = ws[:ws.numel() // 4 * 4].view(torch.float32).cpu().numpy()
    assert (ptr - ws.data_ptr()) % 4 == 0
    return flat[(ptr - ws.data_ptr()) // 4 + R.partial_index(q, n, stride, row_len, row_pitch)]


def _xw_producer(n):
    from gae_dgl_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(n)
    X = torch.randn(n, 200, device=DEV, generator=gen)
    G = torch.randn(n, 16, device=DEV, generator=gen)
    D = torch.randn(n, 16, device=DEV, generator=gen)
    return lambda: ops.xw_wgrad_raw(X, G, None, D, None, 16)


def _linear_producer(n):
    from gae_dgl_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(n)
    dY = torch.randn(n, 4, device=DEV, generator=gen)
    M = torch.randn(n, 8, device=DEV, generator=gen)
    W = torch.randn(4, 8, device=DEV, generator=gen)
    return lambda: ops.linear_bwd_raw(dY, None, ops.ACT_IDENTITY, M, W, need_dM=False)[:2]


def _fused_producer(n):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    rng = np.random.default_rng(n)
    g = G.DGLGraph((rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)), num_nodes=n).to(DEV)
    g.csr(); g.csc()
    gen = torch.Generator(device=DEV).manual_seed(n)
    dY = torch.randn(n, 16, device=DEV, generator=gen)
    W = torch.randn(16, 32, device=DEV, generator=gen) * 0.2
    M = torch.randn(n, 32, device=DEV, generator=gen)
    return lambda: ops.gcn_layer_fused_wgrad_raw(*g.csc(), dY, n, g.spmm_plan(True), W, M, None)[1:]


# row counts: xw_wgrad splits 200 columns into 4 slices and the rows into <= 64 parts of >= 32 rows (dW: one partial
# per part, db: one per part and slice); linear_bwd takes 128 rows per partial; the fused backward 32
@pytest.mark.parametrize("producer,rows", [(_xw_producer, (200, 1000, 1056)), (_linear_producer, (600, 4096, 4100)),
                                           (_fused_producer, (1024, 1056, 2100))],
                         ids=["xw_wgrad", "linear_bwd", "gcn_layer_fused_wgrad"])
def test_stand_alone_reduction_has_the_library_order(producer, rows):
    """the reduction launch of the eager call == adam_ref.sum_in_library_order of the list the same call leaves
    inside deferred_grad_reductions(), bit for bit, for dW and db"""
    from gae_dgl_amd import ops
    lengths = []
    for n in rows:
        call = producer(n)
        with ops.deferred_grad_reductions():
            grads = call()
            entries = [ops.pending_partials(t) for t in grads]        # consumed: the context exits clean
            assert all(e is not None for e in entries)
            torch.cuda.synchronize()
            raw = [_raw_list(e, t.numel()) for e, t in zip(entries, grads)]
        eager = call()
        torch.cuda.synchronize()
        for P, e, t in zip(raw, entries, eager):
            assert P.shape == (e[2], t.numel()) and np.isfinite(P).all()
            assert same_bits(t.reshape(-1).cpu().numpy(), R.sum_in_library_order(P)), (n, e[2:], tuple(t.shape))
            lengths.append(int(e[2]))
    print(f"list lengths {lengths}")
    assert min(lengths) <= 32 < max(lengths), lengths
