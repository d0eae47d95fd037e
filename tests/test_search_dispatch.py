"""GPU tests (-m gpu) of the search dispatch (csrc/nmi_search_plan.h, enqueue_grid / enqueue_grid_mask): one context driven
through alternating kinds of calls, and stream tickets of three kinds around a blocking call.  After every call the scores and
the winner equal the oracle's bit for bit (oracle/binding.py in rounded mode, tests/helpers/masked_np.py, covered_np.py), and
nmi_split_status / nmi_pix_status / nmi_last_content describe THAT call's launch, not an earlier one.  Frames are 64 x 48 and,
for the unaligned-row form, 36 x 20 (a context has one frame size, so that step has a context of its own, interleaved)."""
import numpy as np
import pytest

from helpers import covered_np as cnp
from helpers import masked_np as mnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = 64, 48
W2, H2 = 36, 20


@pytest.fixture(scope="module")
def oc():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    capi.load_library()  # raises if the HIP library is missing: there is no fallback
    from oracle import binding
    return binding


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def noise(n, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def two_levels(n, w, h, seed):
    return np.random.default_rng(seed).choice(np.array([40, 200], np.uint8), (n, h, w))


def masks(n, w, h, seed):
    m = (np.random.default_rng(seed).random((n, h, w)) < 0.85).astype(np.uint8)
    m[:, h - h // 6:] = 0
    return m


def plain_oracle(oc, rs, ws):
    with oc.rounded():
        return oc.search_grid(rs, ws, threads=4)


def status(ctx):
    return (ctx.split_status()["last_launch_parts"], ctx.pix_status()["last_launch_ranges"], ctx.last_content()["few_levels"])


def plain(ctx, oc, rs, ws):
    t = torch.full((ws.shape[0], rs.shape[0]), -3.0, device="cuda")
    idx, best = ctx.search_grid(dev(rs), dev(ws), t)
    ro, io, bo = plain_oracle(oc, rs, ws)
    assert (bits(t.cpu().numpy()) == bits(ro)).all() and (idx, bits(best)) == (io, bits(bo))


def test_alternating_call_kinds_on_one_context(oc):
    """The status after each call, for 256 compute units in automatic mode (tests/native/search_plan.cpp is the table): a pair
    8 row parts, 9 candidates 8, 40 masked candidates 3 pixel ranges, 300 candidates neither, a batch of 5 pairs 8 row parts, 40
    covered candidates on 36-pixel rows 5 pixel ranges.  Two intensities on 9 candidates keep the row-split kernel (few-levels
    flag off); with the split forms switched off the second such search takes the few-levels kernels, and the noise search
    behind it is handed back by its own probe (flag off again)."""
    r1, w1 = noise(1, W, H, 1), noise(1, W, H, 2)
    r3, w3 = noise(3, W, H, 3), noise(3, W, H, 4)
    r8, w5, m5 = noise(8, W, H, 5), noise(5, W, H, 6), masks(5, W, H, 7)
    r20, w15 = noise(20, W, H, 8), noise(15, W, H, 9)
    pr, pw = noise(5, W, H, 10), noise(5, W, H, 11)
    c8, c5, cm5, crm = noise(8, W2, H2, 12), noise(5, W2, H2, 13), masks(5, W2, H2, 14), masks(8, W2, H2, 15)
    crm[:, H2 - H2 // 6:] = 1
    crm[:, :3] = 0
    f3, g3 = two_levels(3, W, H, 16), two_levels(3, W, H, 17)
    with capi.NmiContext(W, H) as ctx, capi.NmiContext(W2, H2) as small:
        full = ctx.info()["compute_units"] == 256

        def after(want, c=ctx):
            got = status(c)
            assert got[2] == want[2], (got, want)
            assert not (got[0] and got[1]), got
            if full:
                assert got == want, (got, want)

        plain(ctx, oc, r1, w1)
        after((8, 0, False))
        plain(ctx, oc, r3, w3)
        after((8, 0, False))

        t = torch.full((5, 8), -3.0, device="cuda")
        idx, best = ctx.search_grid_masked(dev(r8), dev(w5), dev(m5), t)
        mo, mi, mb = mnp.masked_search(r8, w5, m5)
        assert (bits(t.cpu().numpy()) == bits(mo)).all() and (idx, bits(best)) == (mi, bits(mb))
        after((0, 3, False))

        plain(ctx, oc, r20, w15)
        after((0, 0, False))

        dr, dw = dev(pr), dev(pw)
        got = ctx.eval_pairs([dr[i] for i in range(5)], [dw[i] for i in range(5)])
        with oc.rounded():
            want = [oc.eval_pair(pr[i], pw[i]) for i in range(5)]
        assert (bits(got) == bits(want)).all()
        after((8, 0, False))

        t = torch.full((5, 8), -3.0, device="cuda")
        idx, best = small.search_grid_covered(dev(c8), dev(crm), dev(c5), dev(cm5), t)
        co, ci, cb, cc = cnp.covered_search(c8, c5, cm5, crm)
        assert (bits(t.cpu().numpy()) == bits(co)).all() and (idx, bits(best)) == (ci, bits(cb))
        assert (small.cover_counts(40).reshape(5, 8) == cc).all()
        after((0, 5, False), small)
        after((8, 0, False))             # the other context's launch is not this one's

        plain(ctx, oc, f3, g3)
        after((8, 0, False))
        plain(ctx, oc, r3, w3)
        after((8, 0, False))

        ctx.set_option(ctx.OPT_SPLIT, 0)  # one workgroup per candidate: every search is a content probe too
        plain(ctx, oc, f3, g3)
        after((0, 0, False))
        plain(ctx, oc, f3, g3)
        after((0, 0, True))               # the probe before it found 2 x 2 levels
        plain(ctx, oc, r3, w3)
        after((0, 0, False))              # sent the same way, handed back by its own probe
        ctx.set_option(ctx.OPT_SPLIT, -1)
        plain(ctx, oc, r1, w1)
        after((8, 0, False))


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)], ids=["in-order", "reversed"])
def test_stream_tickets_of_three_kinds_around_a_blocking_call(oc, order):
    """Depth 3: a plain 3 x 3, a masked 8 x 5 and a plain 20 x 15 ticket back to back, a blocking search on the same context, then
    the waits in either order: every ticket's winner and kept ratings equal the blocking calls' on the same inputs."""
    K = np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]])
    frames = [noise(1, W, H, 30 + i)[0] for i in range(3)]
    shapes = [(3, (3, 1, 1)), (8, (5, 1, 1)), (20, (5, 3, 1))]
    renders = [noise(S, W, H, 40 + i) for i, (S, _) in enumerate(shapes)]
    Ms = [capi.warp_homographies(K, wc, (0.02, 0.02, 0.05)) for _, wc in shapes]
    rb, wb = noise(3, W, H, 50), noise(3, W, H, 51)
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    with capi.NmiContext(W, H) as ctx:
        with capi.NmiStream(ctx, 20, 15, depth=3) as st:
            st.keep_ratings()
            tickets = [st.submit(pin(renders[0]), pin(frames[0]), Ms[0]),
                       st.submit_masked(pin(renders[1]), pin(frames[1]), None, Ms[1]),
                       st.submit(pin(renders[2]), pin(frames[2]), Ms[2])]
            plain(ctx, oc, rb, wb)       # a blocking search between the submissions and the waits
            got = {}
            for i in order:
                win = st.wait(tickets[i])
                got[i] = (win, st.ratings(tickets[i], len(Ms[i]), shapes[i][0]))
        for i in range(3):
            S, Wn = shapes[i][0], len(Ms[i])
            t = torch.full((Wn, S), -3.0, device="cuda")
            if i == 1:
                ws, wm = ctx.warp_stack_masked(dev(frames[i]), Ms[i])
                win = ctx.search_grid_masked(dev(renders[i]), ws, wm, t)
            else:
                win = ctx.search_grid(dev(renders[i]), ctx.warp_stack(dev(frames[i]), Ms[i]), t)
            assert (got[i][0][0], bits(got[i][0][1])) == (win[0], bits(win[1])), i
            assert (bits(got[i][1]) == bits(t.cpu().numpy())).all(), i
