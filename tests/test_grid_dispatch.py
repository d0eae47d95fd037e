"""GPU tests (-m gpu) of the host side of nmi_grid_kernel's launches: which instantiation <BG, SHIFTED, HIST> launch_grid and
launch_grid_rows pick from (background rule, bins, NMI_OPT_HIST_VARIANT).  The ladder is written once (with_bg_shifted,
csrc/nmi_kernels.h) and every launcher puts its own rule for the exact path inside it, so what can go wrong is an argument in
the wrong place -- and the kernels cannot show that, only a search can: a 3 x 2 grid on the plain kernel (64 x 48, rows of whole
aligned chunks) and on the rows kernel (47 x 33), every cell of background rule x bins x histogram variant, rating table and
winner against the CPU oracle in its rounded term mode, compared with == (tests/test_gpu_parity.py explains the bar).  The
content has zeros in both images and more than 64 grey levels, and the test first checks on the oracle's tables alone that the
four (background rule, bins) settings give four different tables on it: a swapped or dropped argument changes the result."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHIFT = {256: 0, 64: 2}
SHAPES = {"64x48": (48, 64), "47x33": (33, 47)}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stacks(h, w):
    """3 renders and 2 frames: frames are noisy copies of a render (so that scores differ by cell), all 256 grey levels in use,
    and a tenth of the pixels of every image zero, at places of its own."""
    rng = np.random.default_rng(1000 * h + w)
    rs = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    ws = np.stack([np.where(rng.random((h, w)) < 0.6, rs[k], rng.integers(0, 256, (h, w))).astype(np.uint8) for k in (2, 0)])
    for im in list(rs) + list(ws):
        im[rng.random((h, w)) < 0.1] = 0
    return rs, ws


_oracle = {}


def oracle_tables(shape):
    """{(use_bg, bins): (ratings, index, best)} of the shape's stacks, computed once."""
    if shape not in _oracle:
        from oracle import binding as oc
        rs, ws = stacks(*SHAPES[shape])
        with oc.rounded():
            _oracle[shape] = {(bg, bins): oc.search_grid(rs, ws, shift=SHIFT[bins], use_bg=bg, threads=4) for bg in (True, False) for bins in (256, 64)}
    return _oracle[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_content_tells_the_settings_apart(shape):
    """No device: zeros in both stacks, more than 64 grey levels, and four different rating tables for the four settings."""
    rs, ws = stacks(*SHAPES[shape])
    assert (rs == 0).any() and (ws == 0).any() and len(np.unique(rs)) > 64 and len(np.unique(ws)) > 64
    t = oracle_tables(shape)
    keys = list(t)
    for i, a in enumerate(keys):
        assert t[a][0].shape == (2, 3) and np.isfinite(t[a][0]).all() and len(np.unique(bits(t[a][0]))) == 6
        for b in keys[i + 1:]:
            assert (bits(t[a][0]) != bits(t[b][0])).all(), (a, b)


@pytest.mark.parametrize("hist", [3, 1], ids=["hist3", "hist1"])
@pytest.mark.parametrize("bins", [256, 64])
@pytest.mark.parametrize("use_bg", [True, False], ids=["bg", "bgoff"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_cell_of_the_ladder(nmi, shape, use_bg, bins, hist):
    h, w = SHAPES[shape]
    rs, ws = stacks(h, w)
    ro, io, bo = oracle_tables(shape)[(use_bg, bins)]
    with nmi.NmiContext(w, h, bins=bins, use_bg=use_bg) as ctx:
        ctx.set_option(ctx.OPT_SPLIT, 0)
        ctx.set_option(ctx.OPT_HIST_VARIANT, hist)
        t = torch.full((2, 3), -3.0, device="cuda")
        got = ctx.search_grid(torch.from_numpy(rs).cuda(), torch.from_numpy(ws).cuda(), t)
        st = ctx.pix_status(), ctx.split_status()
    assert st[0]["last_launch_ranges"] == 0 and st[1]["last_launch_parts"] == 0, st  # nmi_grid_kernel's own launch
    assert (bits(t.cpu().numpy()) == bits(ro)).all(), (t.cpu().numpy(), ro)
    assert got == (io, bo)
