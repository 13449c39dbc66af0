"""The hash grid's position, ray and scratch-free table gradients ENTRY BY ENTRY against the float64 reference of
tests/position_gradient_reference.py (its docstring derives every bound; tests/test_position_gradient_reference_cpu.py holds a
correct fp32 evaluation and twelve seeded defects to the same bounds), through the C ABI with raw pointers:

* hash_encode_bwd_pos_kernel: `dpositions` of nsamd_hashgrid_encode_bwd / _set at M in {1, 255, 256, 257, 1000} (256 threads per
  block), explicit positions and rays of 5 samples, the three transforms, the 5-level T = 2^12, 8-level T = 2^12 and 16-level
  T = 2^18 grids, denc feature-major, point-major and padded; the same bits with dtable NULL, with dtable and a workspace, with
  dtable and no workspace, and through _set; dtable = dpositions = NULL answers NSAMD_ERR_INVALID_ARG.
* hash_encode_bwd_rays_kernel: d_origins / d_directions of nsamd_hashgrid_encode_bwd_rays and _rays_gated at S in {1, 48, 63, 64,
  65, 130, 256} (the 64-lane strided loop) and n in {1, 3, 4, 5, 257} (four rays per workgroup; every pair on the 5-level grid, a
  covering set of 17 on the 16-level grid), `accumulate` 0 and 1 (fl32(prior + the accumulate = 0 value) bit for bit), the gate
  raised / lowered and a ray mask, and the ray outputs against the float64 reduction of the first kernel's dpositions within the
  sum of both bounds.
* hash_encode_bwd_table_kernel (M = 8191, float atomics) and hash_encode_bwd_sliced_kernel (M = 8192; one slice at T = 2^12, two at
  T = 2^15): nsamd_hashgrid_encode_bwd without a workspace on a zero and a random prefill, _set without one on a NaN-filled table,
  spread points and a batch of identical rays (n_e in the thousands). These sums have no fixed order: only the bound is asserted.
* The module route: functional.table_scatter with dpos and dtable together, and functional.spec_encode under autograd in ray
  mode (torch reduces dpositions per ray: gamma_S on the absolute terms is added to the bound).

Every written buffer starts as NaN between guard rows that must come back intact; every call with a fixed summation order is
issued twice and must give the same bits. No entry is excluded: the reference takes the kernel's branches from the kernel's own
fp32 inputs. No ratio is a pass criterion; the derived bound is.

Worst |err| / bound measured on MI355X over all parametrisations (profiles/hash_position_gradient_float64_ratios.txt; every
test prints its own line, also when an assertion stops it):
  dpositions 0.251 (explicit and 5-sample rays) / 0.275 (the ray shapes): in every case the figure of the host-compiled helpers
  d_origins 0.148   d_directions 0.131   the ray kernel against the float64 sum of the position kernel's output 0.021 / 0.032
  scratch-free table: 0.800 (spread points, a random prefill), 0.001 for the batch of identical rays (n_e about 7000: the bound
  grows like n_e, the error of a correct sum like its root)   module route: dpos 0.251, d_origins 0.095, d_directions 0.098
The first run passed every bound: no kernel was changed. Every bit-equality held (the denc layouts, dtable / workspace / _set,
the raised gate, accumulate = fl32(prior + value), two calls of one shape).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import position_gradient_reference as pg
from float64_check import report

pytestmark = pytest.mark.gpu

F32 = np.float32
OK, ERR_INVALID_ARG = 0, -1
NAN = float("nan")
LAYOUTS = ("feature-major", "point-major", "padded")


@pytest.fixture(scope="module")
def N():
    from nerfstudio_amd import _native

    _native.load()
    return _native


class _Worst(dict):
    title = None


@pytest.fixture
def worst(request):
    """{output: worst |err| / bound} of one test, printed when the test ends, whether or not an assertion stopped it."""
    w = _Worst()
    yield w
    report(f"poshash-f64 gpu {w.title or request.node.name}", w)


class Guarded:
    """n floats on the device (NaN, or `fill`) between two guards of NaN of four rows of `row` floats (256-byte granules)."""

    def __init__(self, n, row, fill=None):
        self.n, self.pad = n, -(-4 * max(row, 1) // 64) * 64
        self.buf = torch.full((n + 2 * self.pad,), NAN, device="cuda")
        if fill is not None:
            self.buf[self.pad : self.pad + n] = torch.from_numpy(np.ascontiguousarray(fill, dtype=F32).reshape(-1)).cuda()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.pad

    def body(self):
        return self.buf[self.pad : self.pad + self.n].cpu().numpy()

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[: self.pad]).all()) and bool(torch.isnan(self.buf[self.pad + self.n :]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


_TABLES = {}


class Dev:
    """A case's inputs on the device and the native structs that point into them."""

    def __init__(self, N, case):
        self.case, self.N = case, N
        key = (case.L, case.log2_T)
        if key not in _TABLES:
            _TABLES[key] = torch.from_numpy(case.table).cuda()
        self.table = _TABLES[key]
        self.grid = N.make_grid(case.L, case.log2_T, case.scal)
        self.box = N.make_aabb(torch.from_numpy(case.box)) if case.transform == pg.XFORM_AABB else N.Aabb()
        if case.rays:
            self.keep = tuple(torch.from_numpy(case.points[k]).cuda() for k in ("origins", "directions", "t_bins"))
            self.pts = N.make_points(None, *self.keep, case.S)
        else:
            self.keep = (torch.from_numpy(case.points["positions"]).cuda(),)
            self.pts = N.make_points(positions=self.keep[0])
        self._denc = {}

    def denc(self, layout):
        """(device tensor, stride_p, stride_k)."""
        if layout not in self._denc:
            c, d = self.case, torch.from_numpy(self.case.denc)
            if layout == "feature-major":
                self._denc[layout] = (d.t().contiguous().cuda(), 1, c.M)
            elif layout == "point-major":
                self._denc[layout] = (d.contiguous().cuda(), 2 * c.L, 1)
            else:  # three NaN columns behind every row
                wide = torch.full((c.M, 2 * c.L + 3), NAN)
                wide[:, : 2 * c.L] = d
                self._denc[layout] = (wide.cuda(), 2 * c.L + 3, 1)
        return self._denc[layout]

    def workspace(self, write_only):
        lib = self.N.load()
        words = int(lib.nsamd_hashgrid_encode_bwd_workspace(self.grid, self.case.M, 1 if write_only else 0))
        if words == 0:
            return None, 0
        state = int(lib.nsamd_hashgrid_encode_bwd_workspace_state(self.grid, self.case.M))
        ws = torch.empty(words, device="cuda")
        ws[:state].zero_()
        return ws, words

    def backward(self, layout, dtable, dpos, ws=None, ws_n=0, write_only=False):
        """nsamd_hashgrid_encode_bwd(_set) -> status; dtable / dpos: raw device addresses or None."""
        lib = self.N.load()
        d, sp, sk = self.denc(layout)
        fn = lib.nsamd_hashgrid_encode_bwd_set if write_only else lib.nsamd_hashgrid_encode_bwd
        rc = fn(self.pts, self.case.M, self.case.transform, self.box, self.N.ptr(self.table), self.grid, self.N.ptr(d), sp, sk,
                dtable, dpos, self.N.ptr(ws), ws_n, self.N.stream())
        torch.cuda.synchronize()
        return rc

    def rays(self, layout, d_o, d_d, accumulate, gate=None, mask=None, gated=False):
        lib = self.N.load()
        d, sp, sk = self.denc(layout)
        args = (self.pts, self.case.M, self.case.transform, self.box, self.N.ptr(self.table), self.grid, self.N.ptr(d), sp, sk, d_o,
                d_d, accumulate)
        if gated:
            rc = lib.nsamd_hashgrid_encode_bwd_rays_gated(*args, None if gate is None else C.cast(gate.data_ptr(), C.c_void_p),
                                                          self.N.ptr(mask), self.N.stream())
        else:
            rc = lib.nsamd_hashgrid_encode_bwd_rays(*args, self.N.stream())
        torch.cuda.synchronize()
        return rc


def _same_bits(a, b):
    return np.array_equal(pg.bits(a).reshape(-1), pg.bits(b).reshape(-1))


def _dpositions(dev, layout, **kw):
    """dpositions of one call shape, issued twice: the same bits, guards intact."""
    M = dev.case.M
    first = None
    for _ in range(2):
        out = Guarded(3 * M, 3)
        assert dev.backward(layout, kw.get("dtable"), out.ptr, kw.get("ws"), kw.get("ws_n", 0), kw.get("write_only", False)) == OK
        assert out.guards_untouched(), f"{dev.case.name} {layout}: dpositions' guards"
        if first is None:
            first = out.body()
        else:
            assert _same_bits(first, out.body()), f"{dev.case.name} {layout}: two calls differ"
    return first.reshape(M, 3)


# ---------------------------------------------------------------- dpositions ------------------------------------------------------
@pytest.mark.parametrize("transform", list(pg.TRANSFORMS))
@pytest.mark.parametrize("grid", list(pg.GRIDS))
def test_dpositions_vs_float64(N, worst, grid, transform):
    tf = pg.TRANSFORMS[transform]
    worst.title = f"dpositions {grid} {transform}"
    L, _, _, log2_T = pg.GRIDS[grid]
    dtable = torch.zeros((L << log2_T) * 2, device="cuda")  # (accumulated into by the call shapes that take one; not read here)
    for M in pg.POS_M:
        for mode in ("positions", "rays") if M % pg.POS_RAY_S == 0 else ("positions",):
            case = pg.position_case(grid, tf, M, mode)
            dev = Dev(N, case)
            got = {layout: _dpositions(dev, layout) for layout in LAYOUTS}
            pg.check_dpositions(case, got["point-major"], worst)
            for layout in LAYOUTS:
                assert _same_bits(got[layout], got["point-major"]), f"{case.name}: dpositions of the {layout} denc"
            ws, ws_n = dev.workspace(False)
            shapes = {"dtable + workspace": dict(dtable=N.ptr(dtable), ws=ws, ws_n=ws_n), "dtable, no workspace": dict(dtable=N.ptr(dtable))}
            ws, ws_n = dev.workspace(True)
            shapes["_set"] = dict(dtable=N.ptr(dtable), ws=ws, ws_n=ws_n, write_only=True)
            shapes["_set, no workspace"] = dict(dtable=N.ptr(dtable), write_only=True)
            for name, kw in shapes.items():
                assert _same_bits(_dpositions(dev, "feature-major", **kw), got["point-major"]), f"{case.name}: dpositions with {name}"


def test_backward_without_an_output_is_an_invalid_argument(N):
    case = pg.position_case("L5-T12", pg.XFORM_CONTRACT, 257)
    dev = Dev(N, case)
    ws = torch.full((1 << 16,), NAN, device="cuda")
    for write_only in (False, True):
        assert dev.backward("point-major", None, None, ws, ws.numel(), write_only) == ERR_INVALID_ARG
        assert bool(torch.isnan(ws).all()), "the workspace was written"
    report("poshash-f64 gpu no output: INVALID_ARG", {"written": 0.0})


# ---------------------------------------------------------------- ray gradients ---------------------------------------------------
def _gate(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def _ray_outputs(dev, layout, accumulate=0, prior=None, **kw):
    """(d_origins, d_directions) [n,3] of one call shape, issued twice on fresh buffers: the same bits, guards intact."""
    n = dev.case.n
    first = None
    for _ in range(2):
        o, d = Guarded(3 * n, 3, None if prior is None else prior[0]), Guarded(3 * n, 3, None if prior is None else prior[1])
        assert dev.rays(layout, o.ptr, d.ptr, accumulate, **kw) == OK
        assert o.guards_untouched() and d.guards_untouched(), f"{dev.case.name}: the ray outputs' guards"
        if first is None:
            first = (o.body().reshape(n, 3), d.body().reshape(n, 3))
        else:
            assert _same_bits(first[0], o.body()) and _same_bits(first[1], d.body()), f"{dev.case.name}: two calls differ"
    return first


@pytest.mark.parametrize("transform", list(pg.TRANSFORMS))
@pytest.mark.parametrize("grid", pg.RAY_GRIDS)
def test_ray_gradients_vs_float64(N, worst, grid, transform):
    tf = pg.TRANSFORMS[transform]
    worst.title = f"ray gradients {grid} {transform}"
    for i, (n, S) in enumerate(pg.RAY_SHAPES[grid]):
        case = pg.ray_case(grid, tf, n, S)
        dev = Dev(N, case)
        layout = LAYOUTS[i % 2]
        d_o, d_d = _ray_outputs(dev, layout)
        pg.check_rays(case, d_o, d_d, worst)
        dpos = _dpositions(dev, layout)
        pg.check_dpositions(case, dpos, worst)
        pg.check_rays_against_dpositions(case, dpos, d_o, d_d, worst)
        rs = np.random.RandomState(n * 1000 + S)
        prior = [(rs.standard_normal((n, 3)) * 10.0 ** rs.uniform(-3, 1, (n, 3))).astype(F32) for _ in range(2)]
        a_o, a_d = _ray_outputs(dev, layout, accumulate=1, prior=prior)
        pg.check_accumulate(f"{case.name} d_origins", prior[0], d_o, a_o)
        pg.check_accumulate(f"{case.name} d_directions", prior[1], d_d, a_d)
        # the gated form: gate raised, no mask = the ungated bits
        g_o, g_d = _ray_outputs(dev, layout, gate=_gate(1), gated=True)
        assert _same_bits(g_o, d_o) and _same_bits(g_d, d_d), f"{case.name}: gate raised"
        g_o, g_d = _ray_outputs(dev, layout, accumulate=1, prior=prior, gate=_gate(1), gated=True)
        assert _same_bits(g_o, a_o) and _same_bits(g_d, a_d), f"{case.name}: gate raised, accumulate"
        # gate 0: exact zeros written / the prior untouched
        z_o, z_d = _ray_outputs(dev, layout, gate=_gate(0), gated=True)
        assert _same_bits(z_o, np.zeros_like(d_o)) and _same_bits(z_d, np.zeros_like(d_d)), f"{case.name}: gate 0"
        z_o, z_d = _ray_outputs(dev, layout, accumulate=1, prior=prior, gate=_gate(0), gated=True)
        assert _same_bits(z_o, prior[0]) and _same_bits(z_d, prior[1]), f"{case.name}: gate 0, accumulate"
        # a ray mask: marked rays carry the ungated bits, the others zero / the prior
        mark = rs.uniform(0, 1, n) < 0.5
        mask = torch.from_numpy(mark.astype(np.uint8)).cuda()
        m_o, m_d = _ray_outputs(dev, layout, gate=_gate(1), mask=mask, gated=True)
        assert _same_bits(m_o, np.where(mark[:, None], d_o, F32(0))) and _same_bits(m_d, np.where(mark[:, None], d_d, F32(0))), \
            f"{case.name}: ray mask"
        m_o, m_d = _ray_outputs(dev, layout, accumulate=1, prior=prior, gate=_gate(1), mask=mask, gated=True)
        assert _same_bits(m_o, np.where(mark[:, None], a_o, prior[0])) and _same_bits(m_d, np.where(mark[:, None], a_d, prior[1])), \
            f"{case.name}: ray mask, accumulate"


def test_ray_gradients_of_explicit_positions_are_an_invalid_argument(N):
    case = pg.position_case("L5-T12", pg.XFORM_CONTRACT, 255)
    dev = Dev(N, case)
    o, d = Guarded(3 * 51, 3), Guarded(3 * 51, 3)
    for gated in (False, True):
        assert dev.rays("point-major", o.ptr, d.ptr, 0, gate=_gate(1) if gated else None, gated=gated) == ERR_INVALID_ARG
        assert o.untouched() and d.untouched()
    report("poshash-f64 gpu ray gradients of explicit positions: INVALID_ARG", {"written": 0.0})


# ---------------------------------------------------------------- scratch-free table paths ----------------------------------------
@pytest.mark.parametrize("batch", ["spread", "identical"])
@pytest.mark.parametrize("M", pg.TABLE_M)
@pytest.mark.parametrize("grid", list(pg.TABLE_GRIDS))
def test_scratch_free_table_gradient_vs_float64(N, worst, grid, M, batch):
    case = pg.table_case(grid, M, batch)
    worst.title = f"scratch-free table {case.name} (largest n_e {int(case.table_reference()[2].max())})"
    dev = Dev(N, case)
    layout = "feature-major" if case.rays else "point-major"
    words = 2 * case.L * case.T
    for kind in ("zero", "random"):
        pre = np.zeros((words,), F32) if kind == "zero" else (np.random.RandomState(5).standard_normal(words) * 1e-3).astype(F32)
        out = Guarded(words, 2, pre)
        assert dev.backward(layout, out.ptr, None) == OK
        assert out.guards_untouched(), f"{case.name}: the table's guards"
        pg.check_table(case, out.body(), pre, worst, name=f"dtable[{kind} prefill]")
    out = Guarded(words, 2)  # NaN-filled: the write-only call must leave a complete table
    assert dev.backward(layout, out.ptr, None, write_only=True) == OK
    assert out.guards_untouched(), f"{case.name}: the table's guards (_set)"
    pg.check_table(case, out.body(), None, worst, name="dtable[_set]")


# ---------------------------------------------------------------- the module route -----------------------------------------------
@pytest.mark.parametrize("transform", list(pg.TRANSFORMS))
def test_module_route_vs_float64(N, worst, transform):
    """functional.table_scatter with dpos and dtable together (the module's cached workspace: the binned scatter), and
    functional.spec_encode under autograd in ray mode: functional._table_and_position_grads -> _position_grads."""
    from nerfstudio_amd import functional as F

    tf = pg.TRANSFORMS[transform]
    worst.title = f"module route {transform}"
    case = pg.position_case("L5-T12", tf, 1000, "rays")
    dev = Dev(N, case)
    spec = F.HashGridSpec(case.L, case.min_res, case.max_res, case.log2_T)
    assert np.array_equal(np.asarray(spec.scalings(), dtype=F32), case.scal)
    d, sp, sk = dev.denc("point-major")
    dpos = torch.full((case.M, 3), NAN, device="cuda")
    dtable = torch.zeros(case.L * case.T, 2, device="cuda")
    F.table_scatter(dev.pts, case.M, tf, dev.box, dev.table, spec, d, sp, sk, dtable, dpos)
    torch.cuda.synchronize()
    pg.check_dpositions(case, dpos.cpu().numpy(), worst)
    assert _same_bits(dpos.cpu().numpy(), _dpositions(dev, "point-major")), "dpositions with and without the table gradient"
    free = Guarded(2 * case.L * case.T, 2, np.zeros(2 * case.L * case.T, F32))
    assert dev.backward("point-major", free.ptr, None) == OK
    pg.check_table(case, free.body(), None, worst, name="dtable[no workspace]")  # (M < 8192: the float-atomic kernel)
    ref = free.body().reshape(-1, 2)
    assert float(np.abs(dtable.cpu().numpy() - ref).max()) <= 2e-5 * float(np.abs(ref).max()), "dtable beside dpos"
    o, dr, t = (x.clone().requires_grad_(r) for x, r in zip(dev.keep, (True, True, False)))
    enc, _ = F.spec_encode(F.PointSpec(None, o, dr, t), dev.table, spec, tf, dev.box)
    enc.backward(d)
    torch.cuda.synchronize()
    pg.check_rays(case, o.grad.cpu().numpy(), dr.grad.cpu().numpy(), worst, extra=pg.torch_reduction_allowance(case))
