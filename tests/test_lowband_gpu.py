"""GPU: the low-band spectral basis (csrc/lowband.hip) — the CSR Laplacian against the dense one, the basis against the
float64 decomposition of the package's own dense Laplacian, its edge cases, that it is a pure function of each cloud, and
the band re-projection against float64 products."""
import numpy as np
import pytest
import torch

from lowband_restatement import ball, face, height_field, sphere, two_blobs

pytestmark = pytest.mark.gpu


def _cf(clouds, dev):
    """list of [N,3] -> [B,3,N] on the device"""
    return torch.from_numpy(np.stack(clouds)).transpose(1, 2).contiguous().to(dev)


def _dense(rowptr, col, val, deg):
    """CSR on the host -> dense float32 [B,N,N], and the check that the columns ascend within every row."""
    rp, co, va, dg = (t.cpu().numpy() for t in (rowptr, col, val, deg))
    B, N = dg.shape
    L = np.zeros((B, N, N), np.float32)
    for b in range(B):
        rows = np.repeat(np.arange(N), np.diff(rp[b]))
        nnz = rp[b, N]
        c = co[b, :nnz]
        assert ((c >= 0) & (c < N)).all() and (c != rows).all()
        same_row = rows[1:] == rows[:-1]
        assert (c[1:][same_row] > c[:-1][same_row]).all(), "columns must ascend within a row"
        L[b, rows, c] = va[b, :nnz]
        L[b, np.arange(N), np.arange(N)] = dg[b]
    return L


def _duplicated(n, seed):
    p = ball(n, seed)
    p[n // 2:n // 2 + n // 4] = p[:n // 4]      # a quarter of the points twice
    return p


CSR_CASES = [("ball", 2, 100), ("tiny", 1, 20), ("sphere", 2, 257), ("face", 1, 1030), ("blobs", 1, 130), ("dup", 1, 100)]


@pytest.mark.parametrize("kind,B,N", CSR_CASES, ids=[f"{k}-{b}x{n}" for k, b, n in CSR_CASES])
def test_csr_laplacian_equals_the_dense_one(ops, dev, kind, B, N):
    gen = dict(ball=ball, tiny=ball, sphere=sphere, face=face, blobs=two_blobs, dup=_duplicated)[kind]
    x = _cf([gen(N, 20 + b) for b in range(B)], dev)
    Ld = ops.graph_laplacian(x, 30, cf=True).cpu().numpy()
    rowptr, col, val, deg = ops.graph_laplacian_csr(x, 30, cf=True)
    assert rowptr.shape == (B, N + 1) and col.shape == val.shape and deg.shape == (B, N)
    Lc = _dense(rowptr, col, val, deg)
    eye = np.eye(N, dtype=bool)[None]
    assert np.array_equal(np.where(eye, 0, Lc), np.where(eye, 0, Ld)), "off-diagonal entries must be the same bits"
    np.testing.assert_allclose(Lc[:, np.arange(N), np.arange(N)], Ld[:, np.arange(N), np.arange(N)], rtol=1e-5)      # n * eps, n <= 80
    assert np.array_equal(Lc, Lc.transpose(0, 2, 1))
    if kind == "tiny":      # k clamps to N: the complete graph
        assert (np.diff(rowptr.cpu().numpy(), axis=1) == N - 1).all()
    # a pure function of the input
    again = ops.graph_laplacian_csr(x, 30, cf=True)
    nnz = int(rowptr[0, N])
    assert torch.equal(again[0], rowptr) and torch.equal(again[3], deg) and torch.equal(again[1][0, :nnz], col[0, :nnz])


def test_csr_capacity_overflow_is_an_error_not_a_truncation(ops, pc3d, dev):
    x = _cf([ball(100, 3)], dev)
    rowptr = ops.graph_laplacian_csr(x, 30, cf=True)[0]
    need = int(rowptr[0, 100])
    ops.graph_laplacian_csr(x, 30, cf=True, capacity=need)
    with pytest.raises(pc3d.Pc3dError, match="capacity"):
        ops.graph_laplacian_csr(x, 30, cf=True, capacity=need - 1)


def _band_reference(L64, adv64, lp):
    w, V = np.linalg.eigh(L64)
    lref = (adv64 @ V[:, :lp]) @ V[:, :lp].T
    gap = (w[lp] - w[lp - 1]) / w[-1] if 0 < lp < len(w) else np.inf
    v32 = torch.linalg.eigh(torch.from_numpy(L64.astype(np.float32)))[1].numpy()[:, :lp]
    a32 = adv64.astype(np.float32)
    return lref, w, gap, np.abs((a32 @ v32) @ v32.T - lref).max()


BASIS_CASES = [(height_field, 64, 8, (3, 13)), (ball, 100, 16, (2, 12)), (two_blobs, 130, 20, (5, 15)), (sphere, 257, 33, (4, 14)),
               (face, 1024, 100, (0,)), (face, 1030, 100, (8,))]


@pytest.mark.parametrize("family,N,lp,seeds", BASIS_CASES, ids=[f"{f.__name__}{n}" for f, n, _, _ in BASIS_CASES])
def test_basis_against_the_float64_decomposition(ops, dev, family, N, lp, seeds):
    """The test matrix is the package's own dense Laplacian (kNN tie-breaks are out of the comparison). The band lfc =
    (adv U) U^T, adv the cloud itself, within max(4 e32, 4e-6 max|adv|) of float64, e32 the error of the fp32 dense
    decomposition; Ritz values, orthonormality and the residual within their bands (figures: DESIGN 3.13)."""
    x = _cf([family(N, s) for s in seeds], dev)
    U, theta, resid = ops.lowband_basis(x, lp, 30, cf=True)
    assert U.shape == (len(seeds), N, lp) and theta.shape == (len(seeds), lp) and resid.shape == (len(seeds),)
    L = ops.graph_laplacian(x, 30, cf=True).cpu().numpy().astype(np.float64)
    lfc, hfc = ops.band_reproject(x, U)
    for b in range(len(seeds)):
        adv = x[b].cpu().numpy().astype(np.float64)
        lref, w, gap, e32 = _band_reference(L[b], adv, lp)
        assert gap >= 2e-4, gap
        Ub = U[b].cpu().numpy().astype(np.float64)
        err = np.abs((adv @ Ub) @ Ub.T - lref).max()
        err_dev = np.abs(lfc[b].cpu().numpy() - lref).max()
        orth = np.abs(Ub.T @ Ub - np.eye(lp)).max()
        print(f"{family.__name__} N={N} lp={lp} seed {seeds[b]}: gap {gap:.1e} e32 {e32:.1e} band error {err:.1e} (ratio "
              f"{err / e32:.2f}; through band_reproject {err_dev:.1e}) orth {orth:.1e} theta "
              f"{np.abs(theta[b].cpu().numpy() - w[:lp]).max():.1e} resid {resid[b].item():.1e} of {1e-5 * w[-1] * np.sqrt(N):.1e}")
        bound = max(4 * e32, 4e-6 * np.abs(adv).max())
        assert err <= bound and err_dev <= bound, (err, err_dev, e32)
        np.testing.assert_allclose(theta[b].cpu().numpy(), w[:lp], rtol=2e-3, atol=2e-4)
        assert orth <= 1e-5
        assert resid[b].item() <= 1e-5 * w[-1] * np.sqrt(N)


def test_full_band_gives_the_cloud_back(ops, dev):
    x = _cf([height_field(64, 3)], dev)
    assert ops.lowband_block(64, 64) == 64
    U, theta, resid = ops.lowband_basis(x, 64)
    lfc, hfc = ops.band_reproject(x, U)
    torch.testing.assert_close(lfc, x, rtol=0, atol=2e-5)
    assert hfc.abs().max().item() <= 2e-5


def test_block_clamps_to_the_cloud(ops, dev):
    assert ops.lowband_block(100, 90) == 100 and ops.lowband_block(1024, 100) == 128 and ops.lowband_block(64, 8) == 36
    x = _cf([ball(100, 2)], dev)
    U, theta, resid = ops.lowband_basis(x, 90)
    Ub = U[0].double().cpu()
    assert (Ub.T @ Ub - torch.eye(90, dtype=torch.float64)).abs().max().item() <= 1e-5
    w = np.linalg.eigvalsh(ops.graph_laplacian(x, 30).cpu().numpy()[0].astype(np.float64))
    np.testing.assert_allclose(theta[0].cpu().numpy(), w[:90], rtol=2e-3, atol=2e-4)


def test_two_components_give_two_zero_ritz_values(ops, dev):
    x = _cf([two_blobs(130, 5)], dev)
    _, theta, _ = ops.lowband_basis(x, 20)
    th = theta[0].cpu().numpy()
    assert np.abs(th[:2]).max() <= 2e-4 and th[2] > 1e-2


def test_low_pass_beyond_the_block_is_refused(ops, dev):
    x = _cf([ball(512, 1)], dev)
    with pytest.raises(ValueError, match=r"128.*full"):
        ops.lowband_basis(x, 120)
    ops.lowband_block(512, 100)


def test_n2048_residual_and_orthonormality(ops, dev):
    """No dense float64 decomposition at this size: the residual is recomputed on the host in float64 from the CSR, the
    bound uses a power iteration's lower estimate of lambda_max (which only tightens it)."""
    N, lp = 2048, 100
    x = _cf([face(N, 5)], dev)
    csr = ops.graph_laplacian_csr(x, 30, cf=True)
    U, theta, resid = ops.lowband_basis_csr(*csr, lp)
    L = _dense(*csr)[0].astype(np.float64)
    Ub, th = U[0].cpu().numpy().astype(np.float64), theta[0].cpu().numpy().astype(np.float64)
    v = np.ones(N) / np.sqrt(N) + 1e-3 * np.cos(np.arange(N))
    for _ in range(60):
        v = L @ v
        v /= np.linalg.norm(v)
    lam = v @ L @ v
    host = np.abs(L @ Ub - Ub * th[None, :]).max()
    orth = np.abs(Ub.T @ Ub - np.eye(lp)).max()
    print(f"N=2048: resid {resid.item():.1e} (host float64 {host:.1e}) of {1e-5 * lam * np.sqrt(N):.1e}, orth {orth:.1e}")
    assert orth <= 1e-5
    assert host <= 1e-5 * lam * np.sqrt(N) and resid.item() <= 1e-5 * lam * np.sqrt(N)
    assert (np.diff(th) >= 0).all()


def test_basis_is_a_pure_function_of_each_cloud(ops, dev):
    clouds = [ball(100, 2), height_field(100, 3), sphere(100, 4)]
    x = _cf(clouds, dev)
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    a = ops.lowband_basis(x, 16)
    b = ops.lowband_basis(x, 16)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), gpu_state)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    for i in range(3):
        alone = ops.lowband_basis(x[i:i + 1].contiguous(), 16)
        for s, t in zip(a, alone):
            assert torch.equal(s[i:i + 1], t), f"cloud {i} of the batch differs from the cloud alone"


@pytest.mark.parametrize("B,N,lp", [(2, 1024, 100), (3, 512, 40), (1, 130, 7), (2, 1000, 96), (1, 1030, 100), (2, 256, 0)])
def test_band_reproject_vs_float64_product(ops, dev, B, N, lp):
    gen = torch.Generator().manual_seed(N + lp)
    q, _ = torch.linalg.qr(torch.randn(B, N, max(lp, 1), generator=gen, dtype=torch.float64))
    adv = torch.randn(B, 3, N, generator=gen, dtype=torch.float64) * 0.4
    U = q[..., :lp].float().contiguous().to(dev)
    a32 = adv.float().contiguous().to(dev)
    lfc, hfc = ops.band_reproject(a32, U)
    U64, a64 = U.double().cpu(), a32.double().cpu()
    co = a64 @ U64
    lref = co @ U64.transpose(1, 2)
    href = a64 - lref
    for got, ref in ((lfc, lref), (hfc, href)):
        err = (got.double().cpu() - ref).abs().max().item()
        assert err <= 1e-5 * max(ref.abs().max().item(), 1.0), (err, ref.abs().max().item())
    torch.testing.assert_close((lfc + hfc).cpu(), a32.cpu(), rtol=0, atol=2e-5)
    # out= buffers (dim-0 slices of a larger one), the coefficients, the sum, and a second call gives the same bits
    big = torch.full((2 * B, 3, N), float("nan"), device=dev)
    h2, c2 = torch.empty_like(a32), torch.empty((B, 3, lp), device=dev)
    ops.band_reproject(a32, U, big[B:], h2, c2, sum=big[:B])
    assert torch.equal(big[B:], lfc) and torch.equal(h2, hfc)
    assert torch.equal(big[:B], lfc + hfc)
    torch.testing.assert_close(c2.double().cpu(), co, rtol=0, atol=1e-5 * max(co.abs().max().item() if lp else 0.0, 1.0))
