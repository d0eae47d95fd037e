"""GPU tests (-m gpu) of nmi_undistort_frame (csrc/nmi_undistort.hip): frame bytes and mask bytes == the numpy twin
(tests/helpers/undistort_np.py) for every coefficient family, frame size (dword and byte stores) and raw mask; zero
coefficients copy the frame; and the float64 tie-distance criterion of tests/test_warp_edges.py on a smooth frame."""
import numpy as np
import pytest

from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy
from test_warp_edges import RHO, noisy_frame, smooth_frame, tap_range

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = [(640, 480), (848, 480), (1241, 376), (333, 97), (17, 5), (1, 1)]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_masks(W, H):
    rng = np.random.default_rng(W * 7 + H)
    return {"none": None, "random": (rng.random((H, W)) < 0.9).astype(np.uint8), "zero": np.zeros((H, W), np.uint8)}


@pytest.mark.parametrize("shape", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_undistort_equals_the_twin(nmi, shape):
    W, H = shape
    K = sy.intrinsics(W, H)
    img = noisy_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        raw = dev(img)
        for fam, coeffs in unp.FAMILIES.items():
            for mname, rm in raw_masks(W, H).items():
                f, m = ctx.undistort_frame(raw, K, coeffs, raw_mask=None if rm is None else dev(rm))
                ef, em = unp.undistort(img, K, coeffs, rm)
                assert (f.cpu().numpy() == ef).all(), (fam, mname, int((f.cpu().numpy() != ef).sum()))
                assert (m.cpu().numpy() == em).all(), (fam, mname, int((m.cpu().numpy() != em).sum()))
                if mname == "zero":
                    assert not m.cpu().numpy().any()
            # without an output mask: the same frame bytes
            f2, none = ctx.undistort_frame(raw, K, coeffs, out_mask=False)
            assert none is None and (f2.cpu().numpy() == unp.undistort(img, K, coeffs)[0]).all()
        if W * H > 1000:
            _, m = ctx.undistort_frame(raw, K, unp.FAMILIES["pincushion"])
            assert 0 < m.cpu().numpy().sum() < W * H  # (the premise: a pincushion lens leaves an invalid border)


@pytest.mark.parametrize("shape", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_zero_coefficients_copy_the_frame(nmi, shape):
    W, H = shape
    img = noisy_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        f, m = ctx.undistort_frame(dev(img), sy.intrinsics(W, H), np.zeros(5))
        assert (f.cpu().numpy() == img).all() and (m.cpu().numpy() == 1).all()
        rm = raw_masks(W, H)["random"]
        _, m = ctx.undistort_frame(dev(img), sy.intrinsics(W, H), np.zeros(5), raw_mask=dev(rm))
        assert (m.cpu().numpy() == rm).all()


def test_odd_output_offsets_take_the_byte_path(nmi):
    """Output rows that do not start on 4-byte boundaries (a frame at an odd offset of a larger buffer): the same bytes."""
    W, H = 64, 16
    K = sy.intrinsics(W, H)
    img = noisy_frame(W, H)
    with nmi.NmiContext(W, H) as ctx:
        big = torch.zeros(W * H + 8, dtype=torch.uint8, device="cuda")
        bigm = torch.zeros(W * H + 8, dtype=torch.uint8, device="cuda")
        out, outm = big[3:3 + W * H].view(H, W), bigm[1:1 + W * H].view(H, W)
        ctx.undistort_frame(dev(img), K, unp.FAMILIES["strong_k3"], out=out, out_mask=outm)
        ef, em = unp.undistort(img, K, unp.FAMILIES["strong_k3"])
        assert (out.cpu().numpy() == ef).all() and (outm.cpu().numpy() == em).all()
        assert not big[:3].any() and not big[3 + W * H:].any() and not bigm[:1].any() and not bigm[1 + W * H:].any()


@pytest.mark.parametrize("family", ["barrel", "pincushion", "tangential", "strong_k3"])
@pytest.mark.parametrize("shape", [(640, 480), (848, 480), (333, 97)], ids=["640x480", "848x480", "333x97"])
def test_float64_criterion(nmi, shape, family):
    """At every pixel whose float64 value lies more than tau(p) = R(p) RHO + 2^-12 from a rounding tie the product's byte is
    the rounded float64 value; elsewhere within 1; fewer than 1 % of the inner pixels are that close to a tie."""
    W, H = shape
    K = sy.intrinsics(W, H)
    img = smooth_frame(W, H)
    coeffs = unp.FAMILIES[family]
    with nmi.NmiContext(W, H) as ctx:
        got = ctx.undistort_frame(dev(img), K, coeffs, out_mask=False)[0].cpu().numpy()
    val = unp.undistort_value_f64(img, K, coeffs)
    ref = np.clip(np.rint(val), 0, 255).astype(int)
    u, v = unp.source_coords_f64((H, W), K, coeffs)
    r, inner = tap_range(img, u, v)
    tau = r * RHO + 2.0 ** -12
    near = np.abs(val - np.floor(val) - 0.5) <= tau
    d = got.astype(int) - ref
    assert np.abs(d).max() <= 1
    assert (d[~near] == 0).all(), int((d[~near] != 0).sum())
    n_in = int(inner.sum())
    assert n_in < 1000 or (near & inner).sum() < 0.01 * n_in
