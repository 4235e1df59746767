"""spgramcf / spgramf against an error bound local to each bin
(tests/spgram_bound.py), past one chunk, one wave and one fold (`-m gpu`).

The float64 reference restates host/spgram.c; outputs are compared in linear
power bin by bin against a bound built from each transform's own window norm,
and the worst ratio must also stay within 4 x the oracle's on the same case
(where psd is the last transform of the tone alone: 4 x the oracle's worst over
the last eight transforms, spgram_bound.margin_oracle).
The streams are a bin-centred tone over a 1e-5 floor (more than 100 dB of
spectrum) and level-1 bursts on the seams of the reduction: the last
transform of a chunk of 64 and the first of the next, the last chunk of a
fold group of 64 and the first of the next, the first transforms of each
call, the final transform.  Rows (spgram_bound.ROWS): the plain path (gather,
batch transform, k_spg_part) at 63 to 2 * 4096 + 67 transforms for
estimate_psd and for accumulate_psd with alpha 0, 0.05 and 1; nfft = 256 and
2048 at 4097 transforms; the fused kernel at nfft = 1024 in all four
instantiations at 255, 256, 257 and 4097 transforms, both modes, the
accumulate stream also cut into calls of exactly 64 transforms, of one and of
none; the fused rows once more through the device entry points on a pointer 8
bytes past a 16-byte boundary.  Then the second launch batch (nfft = 4096, W =
2, 8197 transforms against 8192 per batch), two launches whose batch exceeds
65535 on grid.y, an all-zero stream, and execute() / execute_psd().
"""
import numpy as np
import pytest

import liquidmi as LQ
import spgram_bound as SB

pytestmark = pytest.mark.gpu


def _obj(c):
    return LQ.Spgram(c.nfft, c.window, real_in=c.real)


def _run_dev(c, off=8):
    """The case through accumulate_psd_dev / estimate_psd_dev, the stream `off`
    bytes past a 16-byte boundary."""
    g = _obj(c)
    L = LQ.lib()
    bx = LQ.DeviceBuffer(c.x.nbytes + 32)
    assert bx.p % 16 == 0
    L.liquid_mi355x_memcpy_h2d(bx.p + off, LQ.ptr(c.x), c.x.nbytes)
    if c.mode == "estimate":
        bo = LQ.DeviceBuffer(c.nfft * 4)
        g.estimate_psd_dev(bx.p + off, len(c.x), bo.p)
        g.synchronize()
        return bo.to_array(np.float32, c.nfft)
    pos = 0
    for x, alpha in c.pieces():
        g.accumulate_psd_dev(bx.p + off + pos * c.x.itemsize, len(x), alpha)
        pos += len(x)
    g.synchronize()
    return g.write_accumulation()


@pytest.mark.parametrize("row", SB.ROWS, ids=SB.row_id)
def test_spgram_rows_hold_the_bin_local_bound(row):
    path, levels = SB.row_path(row)
    assert (path == "plain") == (row[2] != 1024) and levels == (2 if row[4] > 4096 else 1)
    c = SB.case(row)
    w = SB.margin_oracle(row, c)
    c.check(SB.run_object(_obj(c), c), w, "%s, %d-level fold" % (path, levels))
    if path != "plain":
        c.check(_run_dev(c), w, "%s, device calls 8 bytes off" % path)


def test_spgram_plain_rows_through_the_device_entry_points():
    """One plain row of each mode on the offset pointer too."""
    for row in (("estimate", False, 64, 48, 4097, None, False, "bursts"),
                ("accumulate", True, 64, 48, 4097, 0.05, True, "bursts")):
        assert row in SB.ROWS
        c = SB.case(row)
        c.check(_run_dev(c), SB.oracle_worst(c), "plain, device calls 8 bytes off")


def test_spgram_all_zero_stream_is_minus_infinity_in_every_bin():
    """As the oracle: 10 log10f(0)."""
    import oracle_lib as O
    for nfft, W, n in ((64, 48, 64 * 16 * 65 + 3), (1024, 512, 256 * 257 + 5)):
        win = SB.kaiser_window(W)
        x = np.zeros(n, np.complex64)
        assert np.all(np.isneginf(O.Spgram(nfft, win).estimate_psd(x)))
        assert np.all(np.isneginf(LQ.Spgram(nfft, win).estimate_psd(x)))


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("nfft,W", [(64, 48), (1024, 301), (1024, 1024), (2048, 301)])
def test_spgram_execute_holds_the_transform_bound(nfft, W, real):
    """execute(): |X - X64| <= d; execute_psd(): 2 |X| d + d^2 + conv(P + 1e-16), a
    tone over the floor, after write() of a stream longer than the window."""
    win = SB.kaiser_window(W)
    w64 = SB.scaled_window(win, nfft)
    x = SB.stream("tone", real, nfft, W, 3 * W + 7)
    g = LQ.Spgram(nfft, win, real_in=real)
    g.write(x[:W + 3])
    g.write(x[W + 3:])
    X64, un = SB._spectra(x, W, w64, nfft, np.array([len(x) - 1]))
    X64, d = X64[0], SB.dfac(nfft) * un[0]
    X = g.execute()
    err = np.max(np.abs(X.astype(np.complex128) - X64))
    print("spgram execute nfft=%d W=%d real=%d: worst %.4g of the bound" % (nfft, W, real, err / d))
    assert np.all(np.isfinite(X.view(np.float32))) and err <= d
    P = np.roll(np.abs(X64) ** 2, nfft // 2) + 1e-16
    bound = np.roll(2 * np.abs(X64) * d + d * d, nfft // 2) + SB.conv(P)
    lin = 10.0 ** (g.execute_psd().astype(np.float64) / 10.0)
    r = np.abs(lin - P) / bound
    print("spgram execute_psd: worst %.4g of the bound at bin %d, span %.1f dB"
          % (np.max(r), np.argmax(r), 10 * np.log10(np.max(P) / np.min(P))))
    assert np.all(np.isfinite(lin)) and np.max(r) <= 1.0


def test_spgram_window_scale_is_the_references():
    for nfft, W in ((64, 48), (1024, 301)):
        win = SB.kaiser_window(W)
        w64 = SB.scaled_window(win, nfft)
        g = LQ.Spgram(nfft, win)
        g.write(np.array([1.0], np.complex64))
        assert np.max(np.abs(np.abs(g.execute()) - w64[-1])) <= 2.0 ** -22 * w64[-1]


# ------------------------------------------------------------------ second batch, launch geometry
def test_spgram_second_launch_batch():
    """nfft = 4096, W = 2: a call of 2^13 + 5 samples is 8197 transforms against
    8192 per launch batch.  The first such call is folded with alpha = 1 (the
    object's first transforms), a second one with alpha = 0.05: the recursion
    crosses the batch seam five transforms from its end."""
    nfft, n = 4096, SB.SECOND_BATCH_N
    assert LQ.spgram_route(False, nfft, 2) == "plain" and LQ.spgram_batch_samples() // nfft == 8192 < n
    win, x, psd, bound, T = SB.two_sample_case(nfft, [(n, 0.3), (n, 0.05)], 5)
    assert T == 2 * n
    g = LQ.Spgram(nfft, win)
    g.accumulate_psd(x[:n], 0.3)
    g.accumulate_psd(x[n:], 0.05)
    SB.check_lin(g.write_accumulation(), psd, bound, "second batch, nfft=4096 W=2 T=2x8197")


def test_spgram_70000_transforms_in_the_gather():
    """nfft = 4, W = 4: estimate_psd of 70000 samples is 70000 transforms, the
    gather's batch on grid.y (capped at 65535 and strided over)."""
    c = SB.gather_case()
    assert c.T == 70000 and LQ.spgram_route(False, 4, 4) == "plain"
    c.check(_obj(c).estimate_psd(c.x), SB.oracle_worst(c), "70000 transforms")


def test_spgram_more_than_65536_chunks():
    """nfft = 2, W = 2: estimate_psd of 2^22 + 2^12 samples is as many
    transforms, 65600 chunks of 64 on k_spg_part's grid.y."""
    c = SB.chunks_case()
    assert c.T == SB.CHUNKS_N and -(-c.T // LQ.spgram_chunk()) > 65536
    c.check(_obj(c).estimate_psd(c.x), SB.oracle_worst(c), "65600 chunks")
