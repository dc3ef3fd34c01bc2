"""GPU tests of the SH colour kernels through the C ABI (splat_sh_colors, splat_sh_colors_backward,
splat_sh_colors_backward_camera: k_sh_colors<DEG, VEC4> of csrc/sh.hip and k_sh_colors_backward<DEG, CAM> of
csrc/splat_grad.hip) against the float64 references and the error measures of tests/sh_ref.py.

Planes.  Every device plane is built as test_gpu_density's _dev builds it: SENT in TAIL words past its end (and before it,
where the plane starts 4 bytes into its buffer), SENT in every word the contract says is not written (an output's rows at and
past n, grad_sh's floats past 3 (degree + 1)^2 in a row), NaN in every input word it says is not read (a row's padding, the
float4s between strided positions, position w).  Every input plane is read back and compared bit for bit.

Bounds.  An accuracy assertion allows the kernel 3 times the worst error of sh_ref's float32 restatement in the same measure on
the same inputs, computed in the test (test_gpu_image_loss's rule: the factor covers FMA contraction and another rounding of
1 / len); tests/test_sh_cpu.py holds the restatement itself within 8 units.  grad_eye keeps test_gpu_ellipsoid_camera_grad's
BOUND.  Every test prints the kernel's figure beside the bound.

What these tests found: the backward decided the clamp on its own sum, contracted to FMAs (splat_grad.hip's build), while the
forward's is not (sh.hip's): test_clamp_edge saw 70 of 3 995 channels the forward kernel had clamped receive a gradient at
degree 1.  The backward now decides on the forward's sums restated with the forward's roundings (sh_forward_sums)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import autograd as AG
from tests import ellipsoid_camera_grad_ref as CR
from tests import sh_ref as SR
from tests.test_gpu_ellipsoid_camera_grad import BOUND as EYE_BOUND

pytestmark = pytest.mark.gpu

SENT = np.uint32(0x7FC0BEEF)  # a quiet NaN with a payload: no kernel arithmetic produces these bits
TAIL = 8
N = 20000
N_EDGES = (0, 1, 63, 64, 65, 255, 256, 257, N)
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def is_zero(a):
    """+-0, bit for bit."""
    return (bits(a) & np.uint32(0x7FFFFFFF)) == 0


def _lib_ctx():
    cx = AG._context(torch.empty(4, device="cuda"))
    return cx.lib, cx.ctx


def _eye_ptr(eye):
    return np.ascontiguousarray(eye, F).ctypes.data_as(C.POINTER(C.c_float))


class Plane:
    """`words` on the device, `offset` words into a 16-byte aligned buffer, SENT before and in the TAIL words past them."""

    def __init__(self, words, offset=0):
        self.words = np.ascontiguousarray(words).view(np.uint32).reshape(-1).copy()
        buf = np.full(offset + self.words.size + TAIL, SENT, np.uint32)
        buf[offset:offset + self.words.size] = self.words
        self.t = torch.from_numpy(buf.view(np.int32)).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.offset = offset
        self.ptr = self.t.data_ptr() + 4 * offset

    def read(self, what):
        raw = self.t.cpu().numpy().view(np.uint32)
        k = self.offset + self.words.size
        assert (raw[:self.offset] == SENT).all() and (raw[k:] == SENT).all(), f"{what}: words outside the plane were written"
        return raw[self.offset:k].copy()

    def unchanged(self, what):
        assert np.array_equal(self.read(what), self.words), f"{what}: an input plane was written"


def filled(words):
    return Plane(np.full(words, SENT, np.uint32))


def takes_vec4(stride, offset_words):
    """splat_sh_colors' rule: float4 rows where the stride is a multiple of 4 floats and the base is 16-byte aligned."""
    return stride % 4 == 0 and (4 * offset_words) % 16 == 0


def strides_of(degree):
    nf = 3 * (degree + 1) ** 2
    return sorted({nf, nf + 1, (nf + 3) // 4 * 4, 48, 52})


def matrix(degree):
    """(sh_stride, sh base offset in words, pos_stride_vec4) cells."""
    return [(s, o, p) for s in strides_of(degree) for o in (0, 1) for p in (1, 3)]


class Inputs:
    """A scene's input planes for one cell: positions (w and the float4s between rows NaN), sh rows (padding NaN), opacity, g."""

    def __init__(self, sc, stride, offset, ps):
        n, nf = sc.n, 3 * sc.nb
        pos = np.full((n * ps, 4), np.nan, F)
        pos[::ps, :3] = sc.pos
        rows = np.full((n, stride), np.nan, F)
        rows[:, :nf] = sc.sh.reshape(n, nf)
        self.pos, self.sh, self.op, self.g = Plane(pos), Plane(rows, offset), Plane(sc.op), Plane(sc.g)
        self.sc, self.stride, self.offset, self.ps = sc, stride, offset, ps

    def unchanged(self):
        for name in ("pos", "sh", "op", "g"):
            getattr(self, name).unchanged(name)


def forward(inp, n=None):
    """color_opacity_out as words (rows, 4) of a plane of the scene's rows, SENT before the call."""
    lib, ctx = _lib_ctx()
    sc = inp.sc
    n = sc.n if n is None else n
    out = filled(4 * sc.n)
    rc = lib.splat_sh_colors(ctx, _eye_ptr(sc.eye), inp.pos.ptr, inp.ps, inp.sh.ptr, inp.stride, sc.degree, inp.op.ptr, n, out.ptr)
    assert rc == 0, lib.splat_last_error(ctx)
    torch.cuda.synchronize()
    inp.unchanged()
    return out.read("color_opacity_out").reshape(sc.n, 4)


def backward(inp, camera, n=None, null_opacity=False):
    """dict of words: grad_sh (rows, stride), grad_positions (rows, 4), grad_opacity (rows,), grad_eye (4,) or None."""
    lib, ctx = _lib_ctx()
    sc = inp.sc
    n = sc.n if n is None else n
    gsh, gp, gop, ge = Plane(np.full(sc.n * inp.stride, SENT, np.uint32), inp.offset), filled(4 * sc.n), filled(sc.n), filled(4)
    args = (ctx, _eye_ptr(sc.eye), inp.pos.ptr, inp.ps, inp.sh.ptr, inp.stride, sc.degree, None if null_opacity else inp.op.ptr, inp.g.ptr, n,
            gsh.ptr, gp.ptr, gop.ptr)
    rc = lib.splat_sh_colors_backward_camera(*args, ge.ptr) if camera else lib.splat_sh_colors_backward(*args)
    assert rc == 0, lib.splat_last_error(ctx)
    torch.cuda.synchronize()
    inp.unchanged()
    return dict(grad_sh=gsh.read("grad_sh").reshape(sc.n, inp.stride), grad_positions=gp.read("grad_positions").reshape(sc.n, 4),
                grad_opacity=gop.read("grad_opacity"), grad_eye=ge.read("grad_eye") if camera else None)


@functools.lru_cache(maxsize=None)
def reference(degree):
    """The scene of N rows and everything computed from it on the CPU, once for all tests (none of them changes it)."""
    sc = SR.scene(degree, N, 7)
    c64, c32 = SR.colors64(sc), SR.forward32(sc)
    passed = c32[:, :3] > 0
    assert np.array_equal(passed, c64[:, :3] > 0)  # (scene() keeps every channel EDGE_GAP units from the edge)
    gsh64, gp64, _ = SR.backward64(sc, passed)
    gsh32, gp32 = SR.backward32(sc, passed)
    bound = dict(color=3 * float(SR.color_units(sc, c32, c64).max()), grad_sh=3 * float(SR.grad_sh_units(sc, gsh32, gsh64, passed).max()),
                 grad_positions=3 * float(SR.grad_pos_units(sc, gp32, gp64, passed).max()))
    return dict(sc=sc, c64=c64, passed=passed, gsh64=gsh64, gp64=gp64, bound=bound)


def check_backward_accuracy(sc, got, gsh64, gp64, passed, bound, label):
    """grad_sh and grad_positions (words) within the bounds; returns the two figures."""
    nf = 3 * sc.nb
    gsh = got["grad_sh"][:, :nf].view(F).reshape(sc.n, sc.nb, 3)
    gp = got["grad_positions"].view(F)
    assert np.isfinite(gsh).all() and np.isfinite(gp).all(), f"{label}: a gradient is not finite"
    assert (got["grad_positions"][:, 3] == 0).all(), f"{label}: grad_positions w is not 0"
    e_s = float(SR.grad_sh_units(sc, gsh, gsh64, passed).max())
    e_p = float(SR.grad_pos_units(sc, gp, gp64, passed).max())
    assert e_s <= bound["grad_sh"], f"{label}: grad_sh {e_s:.3g} units of 2^-24, bound {bound['grad_sh']:.3g}"
    assert e_p <= bound["grad_positions"], f"{label}: grad_positions {e_p:.3g} units of 2^-24, bound {bound['grad_positions']:.3g}"
    return e_s, e_p


# ---- (a) the forward on every load path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_forward_every_load_path(device, degree):
    """sh_stride in {nf, nf + 1, nf rounded up to 4, 48, 52} x sh base 0 or 4 bytes into its buffer x pos_stride_vec4 1 or 3.
    The cells with a stride that is a multiple of 4 AND base offset 0 take k_sh_colors<degree, VEC4 = true> (at degree 0 and 2
    it loads one float more than the row holds, from inside the stride: a NaN here); all others the scalar loads.  Every cell
    gives the same bits, within the bound of float64, finite, the opacity passed through bit for bit, guards untouched."""
    R = reference(degree)
    sc, bound = R["sc"], R["bound"]["color"]
    first, paths, worst = None, {True: 0, False: 0}, 0.0
    for stride, offset, ps in matrix(degree):
        label = f"degree {degree} stride {stride} offset {4 * offset} B pos_stride {ps}"
        paths[takes_vec4(stride, offset)] += 1
        out = forward(Inputs(sc, stride, offset, ps))
        col = out.view(F)
        assert np.isfinite(col).all(), f"{label}: a colour is not finite"
        assert np.array_equal(out[:, 3], bits(sc.op)), f"{label}: the opacity is not passed through"
        e = float(SR.color_units(sc, col, R["c64"]).max())
        worst = max(worst, e)
        assert e <= bound, f"{label}: colour {e:.3g} units of 2^-24, bound {bound:.3g}"
        first = out if first is None else first
        assert np.array_equal(out, first), f"{label}: differs from the first cell in {int((out != first).any(axis=1).sum())} rows"
    print(f"forward degree {degree}: colour {worst:.3g} units of 2^-24 (bound {bound:.3g}); {paths[True]} VEC4 and {paths[False]} scalar cells, bit-equal")
    assert paths[True] >= 1 and paths[False] >= 1, "a load path has no cell"


# ---- (b) the edges of n ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 3])
def test_n_edges(device, degree):
    """n at the wave's and the workgroup's edges, on a VEC4 and a scalar stride, for the three entry points: nothing written at or
    past row n, rows < n bit-equal to the N-row call's (one lane per splat: no row depends on n), grad_eye within BOUND
    (relative L2 over xyz) of the float64 sum, +-0 at degree 0, zeros for n = 0."""
    R = reference(degree)
    sc = R["sc"]
    nf = 3 * sc.nb
    worst = 0.0
    scalar_stride = nf + 1 if (nf + 1) % 4 else nf + 2
    assert takes_vec4((nf + 3) // 4 * 4, 0) and not takes_vec4(scalar_stride, 0)
    for stride, ps in (((nf + 3) // 4 * 4, 1), (scalar_stride, 3)):
        inp = Inputs(sc, stride, 0, ps)
        full_f, full_b = forward(inp), backward(inp, False)
        for n in N_EDGES:
            label = f"degree {degree} stride {stride} n={n}"
            out = forward(inp, n)
            assert (out[n:] == SENT).all(), f"{label}: color_opacity_out written at or past row n"
            assert np.array_equal(out[:n], full_f[:n]), f"{label}: a colour depends on n"
            for camera in (False, True):
                got = backward(inp, camera, n)
                for name in ("grad_sh", "grad_positions", "grad_opacity"):
                    assert (got[name][n:] == SENT).all(), f"{label} camera={camera}: {name} written at or past row n"
                    assert np.array_equal(got[name][:n], full_b[name][:n]), f"{label} camera={camera}: {name} depends on n"
                assert (got["grad_sh"][:, nf:] == SENT).all(), f"{label} camera={camera}: grad_sh written past 3 (degree + 1)^2 in a row"
            ge = got["grad_eye"]
            assert ge[3] == 0, f"{label}: grad_eye w"
            if degree == 0 or n == 0:
                assert is_zero(ge[:3]).all() and (n > 0 or (ge == 0).all()), f"{label}: grad_eye {ge.view(F)}"
                continue
            want = SR.grad_eye64(sc.rows(n), R["passed"][:n])
            e = CR.rel_l2(ge[:3].view(F), want)
            worst = max(worst, e)
            assert e <= EYE_BOUND, f"{label}: grad_eye relative L2 {e:.3g}"
    print(f"n edges degree {degree}: worst grad_eye relative L2 {worst:.3g} (bound {EYE_BOUND:.3g})")


# ---- (c) the backward on the same matrix -------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_backward_every_stride(device, degree):
    """(a)'s matrix for both backward entry points (grad_sh has sh's stride and base offset).  grad_sh's floats past nf in a row
    keep SENT; every cell gives the same bits, the camera variant the plain one's; grad_sh and grad_positions within the bounds,
    the clamp held at the float32 forward's decisions (float64's: scene() keeps the channels off the edge); grad_opacity is
    g[:, 3] bit for bit, with opacity_f32 = NULL too; no input is written."""
    R = reference(degree)
    sc, nf = R["sc"], 3 * R["sc"].nb
    first, worst = None, np.zeros(2)
    for stride, offset, ps in matrix(degree):
        inp = Inputs(sc, stride, offset, ps)
        for camera in (False, True):
            label = f"degree {degree} stride {stride} offset {4 * offset} B pos_stride {ps} camera={camera}"
            got = backward(inp, camera)
            assert (got["grad_sh"][:, nf:] == SENT).all(), f"{label}: grad_sh written past 3 (degree + 1)^2 in a row"
            assert np.array_equal(got["grad_opacity"], bits(sc.g[:, 3])), f"{label}: grad_opacity is not g[:, 3]"
            worst = np.maximum(worst, check_backward_accuracy(sc, got, R["gsh64"], R["gp64"], R["passed"], R["bound"], label))
            first = got if first is None else first
            for name in ("grad_positions", "grad_opacity"):
                assert np.array_equal(got[name], first[name]), f"{label}: {name} differs from the first cell"
            assert np.array_equal(got["grad_sh"][:, :nf], first["grad_sh"][:, :nf]), f"{label}: grad_sh differs from the first cell"
        if first.get("null") is None:
            first["null"] = backward(inp, False, null_opacity=True)
            for name in ("grad_positions", "grad_opacity", "grad_sh"):
                assert np.array_equal(first["null"][name], first[name]), f"degree {degree}: {name} with opacity_f32 = NULL"
    clamped = ~R["passed"]
    gsh = first["grad_sh"][:, :nf].reshape(sc.n, sc.nb, 3)
    assert clamped.any() and is_zero(gsh.transpose(0, 2, 1)[clamped]).all()
    print(f"backward degree {degree}: grad_sh {worst[0]:.3g} units of 2^-24 (bound {R['bound']['grad_sh']:.3g}), grad_positions {worst[1]:.3g} "
          f"(bound {R['bound']['grad_positions']:.3g}); {2 * len(matrix(degree))} calls bit-equal")


# ---- (d) the clamp's edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_clamp_edge(device, degree):
    """Channels within a few roundings of max(., 0)'s edge (sh_ref.edge_scene; at least 200 on each side within 4 colour units,
    or the test fails).  The backward's decisions are the forward KERNEL's: where color_opacity_out is exactly 0 the channel's
    grad_sh column is +-0, and grad_sh and grad_positions are within the bounds of the float64 reference whose clamp is held
    at `color_opacity_out > 0` (a consistency check between two kernels, as test_gpu_grad_decisions makes for the composite; the
    bound is the restatement's under the same mask).  Where the float64 colour is farther from 0 than the colour bound the
    kernel's decision is float64's.  VEC4 and scalar loads give the same bits here too."""
    sc = SR.edge_scene(degree, 11)
    above, below = SR.edge_counts(sc)
    assert above >= 200 and below >= 200, f"degree {degree}: {above} channels above the edge, {below} below it"
    nf = 3 * sc.nb
    inp = Inputs(sc, 48, 0, 1)
    out = forward(inp)
    assert takes_vec4(48, 0) and np.array_equal(forward(Inputs(sc, nf + 1, 1, 3)), out), "VEC4 and scalar loads differ"
    col = out.view(F)
    c64, c32 = SR.colors64(sc), SR.forward32(sc)
    cb = 3 * float(SR.color_units(sc, c32, c64).max())
    e_c = float(SR.color_units(sc, col, c64).max())
    assert np.isfinite(col).all() and e_c <= cb, f"degree {degree}: colour {e_c:.3g} units of 2^-24, bound {cb:.3g}"
    live = col[:, :3] > 0
    dist = SR.edge_distance_units(sc)
    decided = np.abs(dist) > cb
    assert np.array_equal(live[decided], dist[decided] > 0), f"degree {degree}: a clamp decision differs from float64's beyond the colour bound"
    gsh64, gp64, _ = SR.backward64(sc, live)
    gsh32, gp32 = SR.backward32(sc, live)
    bound = dict(grad_sh=3 * float(SR.grad_sh_units(sc, gsh32, gsh64, live).max()), grad_positions=3 * float(SR.grad_pos_units(sc, gp32, gp64, live).max()))
    for camera in (False, True):
        got = backward(inp, camera)
        gsh = got["grad_sh"][:, :nf].reshape(sc.n, sc.nb, 3)
        wrong = ~is_zero(gsh.transpose(0, 2, 1)[~live]).all(axis=1)
        assert not wrong.any(), f"degree {degree} camera={camera}: {int(wrong.sum())} channels the forward kernel clamped have a gradient"
        e_s, e_p = check_backward_accuracy(sc, got, gsh64, gp64, live, bound, f"degree {degree} camera={camera}")
    zero32 = int((SR.sums32(sc) == 0).sum())
    print(f"clamp edge degree {degree}: {sc.n} rows, {above} / {below} channels above / below the edge within 4 units, {int((~live).sum())} clamped by the "
          f"kernel, {int((~decided).sum())} within the colour bound, {zero32} binary32 sums exactly 0; colour {e_c:.3g} (bound {cb:.3g}), grad_sh "
          f"{e_s:.3g} (bound {bound['grad_sh']:.3g}), grad_positions {e_p:.3g} (bound {bound['grad_positions']:.3g}) units of 2^-24")


# ---- (e) the torch Functions ---------------------------------------------------------------------------------------------------
def _run_sh_colors(sc, make_sh, degree):
    """(colours, dL/dmeans, dL/dsh (n, K, 3), dL/dopacity) as words, of AG.sh_colors on make_sh(the (n, K, 3) leaf)."""
    means = torch.tensor(sc.pos, device="cuda", requires_grad=True)
    opac = torch.tensor(sc.op, device="cuda", requires_grad=True)
    leaf = torch.tensor(sc.sh, device="cuda", requires_grad=True)  # (n, K, 3)
    col = AG.sh_colors(sc.eye, means, make_sh(leaf), degree, opac)
    (col * torch.tensor(sc.g, device="cuda")).sum().backward()
    torch.cuda.synchronize()
    return tuple(bits(t.detach().cpu().numpy()) for t in (col, means.grad, leaf.grad, opac.grad))


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_sh_colors_of_a_higher_degree_plane(device, degree):
    """AG.sh_colors at degree 0-2 on an (n, 16, 3) plane (stride 48, 3DGS's progressive-degree schedule): the colours and the
    gradients of bands <= degree are the compact (n, nb, 3) call's bits, the gradient of every higher band exact zeros."""
    sc16 = SR.scene(3, 5000, 9)
    nb = (degree + 1) ** 2
    compact = SR.Scene(degree, sc16.eye, sc16.pos, np.ascontiguousarray(sc16.sh[:, :nb]), sc16.op, sc16.g)
    a = _run_sh_colors(sc16, lambda t: t, degree)
    b = _run_sh_colors(compact, lambda t: t, degree)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[2][:, :nb], b[2]), "a band's gradient differs from the compact call's"
    assert (a[2][:, nb:] == 0).all(), "a band above the degree has a gradient"
    assert a[2][:, :nb].any() and np.array_equal(a[3], bits(sc16.g[:, 3]))


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_colors_layouts_and_update_colors(device, degree):
    """A non-contiguous sh (a permuted view of (n, 3, K) storage) and an (n, 3K) reshape give the (n, K, 3) call's bits, which
    are the ABI call's; GaussianCloud.updateColors gives them too."""
    sc = reference(degree)["sc"].rows(5000)
    base = _run_sh_colors(sc, lambda t: t, degree)
    permuted = _run_sh_colors(sc, lambda t: t.permute(0, 2, 1).contiguous().permute(0, 2, 1), degree)
    flat = _run_sh_colors(sc, lambda t: t.reshape(sc.n, -1), degree)
    for other in (permuted, flat):
        assert all(np.array_equal(x, y) for x, y in zip(base, other))
    inp = Inputs(sc, 3 * sc.nb, 0, 1)
    abi_f, abi_b = forward(inp), backward(inp, False)
    assert np.array_equal(base[0], abi_f)
    assert np.array_equal(base[1], abi_b["grad_positions"][:, :3]) and np.array_equal(base[2].reshape(sc.n, -1), abi_b["grad_sh"])
    rot = np.tile(np.array([1, 0, 0, 0], F), (sc.n, 1))
    cloud = sr.GaussianCloud.fromArrays(device, sc.pos, np.full((sc.n, 3), 0.01, F), rot, opacity=sc.op, sh=sc.sh)
    assert cloud.shDegree == degree
    cloud.updateColors(sc.eye)
    got = cloud.colorOpacity.read(np.uint32).reshape(sc.n, 4)
    cloud.destroy()
    assert np.array_equal(got, abi_f), "GaussianCloud.updateColors differs from the ABI call"


def test_sh_colors_of_no_splats(device):
    """n = 0: empty tensors, empty gradients, and a zero gradient for an eye that requires one."""
    for degree in (0, 3):
        nb = (degree + 1) ** 2
        means = torch.zeros((0, 3), device="cuda", requires_grad=True)
        sh = torch.zeros((0, nb, 3), device="cuda", requires_grad=True)
        op = torch.zeros(0, device="cuda", requires_grad=True)
        eye = torch.tensor(SR.EYE.astype(np.float64), requires_grad=True)
        col = AG.sh_colors(eye, means, sh, degree, op)
        assert col.shape == (0, 4)
        col.sum().backward()
        assert means.grad.shape == (0, 3) and sh.grad.shape == (0, nb, 3) and op.grad.shape == (0,)
        assert eye.grad.shape == (3,) and not eye.grad.any()


# ---- (f) refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(device):
    """What include/splat.h says is refused, on the three entry points: sh or opacity_f32 off by 2 bytes, a vec4 plane off by 4,
    pos_stride_vec4 = 0, degree 4, sh_stride below 3 (degree + 1)^2.  n = 0 with NULL planes is accepted.  Nothing is launched by
    a refused call: the output planes keep SENT."""
    lib, ctx = _lib_ctx()
    sc = reference(1)["sc"].rows(64)
    inp = Inputs(sc, 12, 0, 1)
    eye = _eye_ptr(sc.eye)
    out, gsh, gp, gop, ge = filled(4 * sc.n), filled(12 * sc.n), filled(4 * sc.n), filled(sc.n), filled(4)

    def fwd(pos=inp.pos.ptr, ps=1, sh=inp.sh.ptr, stride=12, degree=1, op=inp.op.ptr, n=sc.n, o=out.ptr):
        return lib.splat_sh_colors(ctx, eye, pos, ps, sh, stride, degree, op, n, o)

    def bwd(camera, pos=inp.pos.ptr, ps=1, sh=inp.sh.ptr, stride=12, degree=1, op=inp.op.ptr, g=inp.g.ptr, n=sc.n, gs=gsh.ptr, p=gp.ptr, o=gop.ptr,
            e=ge.ptr):
        args = (ctx, eye, pos, ps, sh, stride, degree, op, g, n, gs, p, o)
        return lib.splat_sh_colors_backward_camera(*args, e) if camera else lib.splat_sh_colors_backward(*args)

    assert fwd(sh=inp.sh.ptr + 2) == -1 and fwd(op=inp.op.ptr + 2) == -1
    assert fwd(pos=inp.pos.ptr + 4) == -1 and fwd(o=out.ptr + 4) == -1
    assert fwd(ps=0) == -1 and fwd(degree=4, stride=75) == -1 and fwd(stride=11) == -1
    for camera in (False, True):
        assert bwd(camera, sh=inp.sh.ptr + 2) == -1 and bwd(camera, op=inp.op.ptr + 2) == -1
        assert bwd(camera, pos=inp.pos.ptr + 4) == -1
        assert bwd(camera, ps=0) == -1 and bwd(camera, degree=4, stride=75) == -1 and bwd(camera, stride=11) == -1
    assert bwd(True, e=ge.ptr + 4) == -1
    torch.cuda.synchronize()
    for name, p in (("color_opacity_out", out), ("grad_sh", gsh), ("grad_positions", gp), ("grad_opacity", gop), ("grad_eye", ge)):
        assert (p.read(name) == SENT).all(), f"a refused call wrote {name}"
    assert lib.splat_sh_colors(ctx, eye, None, 1, None, 12, 1, None, 0, None) == 0
    assert lib.splat_sh_colors_backward(ctx, eye, None, 1, None, 12, 1, None, None, 0, None, None, None) == 0
    assert lib.splat_sh_colors_backward_camera(ctx, eye, None, 1, None, 12, 1, None, None, 0, None, None, None, ge.ptr) == 0
    torch.cuda.synchronize()
    assert (ge.read("grad_eye") == 0).all(), "n = 0 does not write the zeros to grad_eye"
    # and the accepted call still works after the refusals
    assert fwd() == 0 and bwd(False) == 0 and bwd(True) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.read("color_opacity_out").reshape(sc.n, 4), forward(inp))
