"""The s3 NT register epilogue rolled into the last k chunk (gemm_s3.hip, DIRECT without dropout)
against the LDS epilogue of the same product: the same A and B run both ways by the choice of ldc
(ldc % 4 == 0 takes the register epilogue, else the LDS one), compared bit for bit, and against an
fp64 product at the s3 kernels' 2e-6 relative bound so that a fault common to both cannot pass.

Shapes: M = 257 / 300 (a ragged last row tile), N = 400 (two column tiles, the second one's last
fragment dead) / 212 (a second tile with one live 4-column piece), K = 416 / 432 (a whole / half
last chunk; 13 / 14 chunks: the last chunk is the odd / even step of the loop's pairs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from deep_learning_amd import _lib  # noqa: E402
from deep_learning_amd._lib import call, ptr  # noqa: E402

SHAPES = [(257, 400, 416), (300, 400, 432), (300, 212, 416), (257, 212, 432)]
LDBITS = 32   # even, and wide enough for the register bitmask epilogue's seven dwords a tile


def _s():
    return _lib.stream_handle()


def _planes(W):
    """dl_split3 planes of the f32 matrix W [N][K] as int16 [3][N][K]."""
    rows, cols = W.shape
    P = torch.zeros(3 * rows * cols, dtype=torch.int16, device="cuda")
    call("dl_split3", ptr(W), rows, cols, cols, 0, ptr(P), cols, rows * cols, _s())
    return P


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(M, K + 4)
    A[:, :K] = torch.randn(M, K, generator=g)
    Bm = torch.randn(N, K, generator=g) * 0.05
    ref = A[:, :K].double() @ Bm.double().t()
    scale = (A[:, :K].abs().double() @ Bm.abs().double().t()).clamp(min=1e-3)
    bits = torch.randint(-32768, 32768, (M, LDBITS), generator=g, dtype=torch.int32).to(torch.int16)
    return A.cuda(), Bm.cuda(), ref, scale, bits.cuda()


def _unpack(bits, N):
    """[M][ldbits] halfwords -> [M][N] bool (bit c & 15 of halfword c >> 4)."""
    nh = (N + 15) // 16
    words = bits[:, :nh].to(torch.int32) & 0xFFFF
    return ((words[:, :, None] >> torch.arange(16, device=bits.device)) & 1).reshape(bits.shape[0], nh * 16)[:, :N].bool()


def _run(M, N, K, A, Bp, epi, ldc, bits):
    C = torch.full((M, ldc), 7.0, device="cuda")
    call("dl_gemm_s3_nt_bits", M, N, K, ptr(A), K + 4, ptr(Bp), K, N * K, ptr(C), ldc, epi, None, 0,
         ptr(bits), LDBITS if bits is not None else 0, _s())
    torch.cuda.synchronize()
    return C


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_rolled_epilogue_bit_identical_to_lds_epilogue(hip_lib, M, N, K):
    A, Bm, ref, scale, rnd = _operands(M, N, K, M + 3 * N + K)
    Bp = _planes(Bm)
    err = lambda C, want: ((C[:, :N].double().cpu() - want).abs() / scale).max().item()
    # store
    c_reg, c_lds = _run(M, N, K, A, Bp, 0, N + 4, None), _run(M, N, K, A, Bp, 0, N + 3, None)
    assert torch.equal(c_reg[:, :N], c_lds[:, :N])
    assert (c_reg[:, N:] == 7.0).all() and (c_lds[:, N:] == 7.0).all()
    e = err(c_reg, ref)
    print("store    M %d N %d K %d: rel err %.3e" % (M, N, K, e))
    assert e < 2e-6
    # ReLU with the sign bitmask: the output and the halfwords
    b_reg = torch.full((M, LDBITS), -1, dtype=torch.int16, device="cuda")
    b_lds = torch.full((M, LDBITS), -1, dtype=torch.int16, device="cuda")
    h_reg, h_lds = _run(M, N, K, A, Bp, 1, N + 4, b_reg), _run(M, N, K, A, Bp, 1, N + 3, b_lds)
    assert torch.equal(h_reg[:, :N], h_lds[:, :N])
    assert (h_reg[:, N:] == 7.0).all()
    assert torch.equal(b_reg, b_lds)
    assert (b_reg[:, (N + 15) // 16:] == -1).all()
    assert torch.equal(_unpack(b_reg, N), h_reg[:, :N] > 0)
    e = err(h_reg, ref.clamp(min=0))
    print("relu     M %d N %d K %d: rel err %.3e" % (M, N, K, e))
    assert e < 2e-6
    # ReluGrad from a random bitmask
    d_reg, d_lds = _run(M, N, K, A, Bp, 3, N + 4, rnd), _run(M, N, K, A, Bp, 3, N + 3, rnd)
    assert torch.equal(d_reg[:, :N], d_lds[:, :N])
    assert (d_reg[:, N:] == 7.0).all()
    keep = _unpack(rnd, N).cpu()
    e = err(d_reg, torch.where(keep, ref, torch.zeros_like(ref)))
    print("maskbits M %d N %d K %d: rel err %.3e" % (M, N, K, e))
    assert e < 2e-6
    assert (d_reg[:, :N].cpu()[~keep] == 0).all()


@pytest.mark.parametrize("M,N,K,F,E", [(300, 400, 432, 26, 16), (257, 212, 72, 8, 8)])
def test_rolled_training_gather_equals_lookup_then_gemm(hip_lib, M, N, K, F, E):
    """dl_gemm_s3_nt_gather_rows (the training form: the first layer gathers x0's deep columns from
    the row buffer and the column-tile-0 blocks write them to x0) with more than one column tile,
    a batch that is no multiple of 256 and negative indices: C, the bitmask and x0's deep columns
    against a lookup followed by the LDS-epilogue GEMM, bit for bit."""
    g = torch.Generator().manual_seed(M + N + K + F)
    n_rows, base = 3000, 5
    rows = torch.randn(n_rows, E, generator=g)
    idx = torch.randint(0, n_rows - base, (M, F + 1), generator=g, dtype=torch.int32)
    idx[::7, 0] = -1
    idx[3::13, F // 2] = -9
    idx[5::11, F - 1] = -1
    take = (idx[:, :F].long() + base).clamp(0, n_rows - 1)
    look = rows[take] * (idx[:, :F] >= 0)[:, :, None]
    x0_ref = torch.zeros(M, K + 4)
    x0_ref[:, F * E:K] = torch.randn(M, K - F * E, generator=g)
    x0 = x0_ref.clone()
    x0_ref[:, :F * E] = look.reshape(M, F * E)
    x0[:, :F * E] = float("nan")   # written by the kernel, never read
    Bm = (torch.randn(N, K, generator=g) * 0.05).cuda()
    Bp = _planes(Bm)
    ref = x0_ref[:, :K].double() @ Bm.double().cpu().t()
    scale = (x0_ref[:, :K].abs().double() @ Bm.abs().double().cpu().t()).clamp(min=1e-3)
    xr, rd, id_ = x0_ref.cuda(), rows.cuda(), idx.cuda()
    for epi in (1, 0):
        b_lds = torch.full((M, LDBITS), -1, dtype=torch.int16, device="cuda") if epi == 1 else None
        b = torch.full((M, LDBITS), -1, dtype=torch.int16, device="cuda") if epi == 1 else None
        c_lds = _run(M, N, K, xr, Bp, epi, N + 3, b_lds)
        xd = x0.cuda()
        c = torch.full((M, N + 4), 7.0, device="cuda")
        call("dl_gemm_s3_nt_gather_rows", M, N, K, ptr(xd), K + 4, ptr(rd), n_rows, E, ptr(id_), F + 1, base, F, E,
             ptr(Bp), K, N * K, ptr(c), N + 4, epi, ptr(b), LDBITS if epi == 1 else 0, _s())
        torch.cuda.synchronize()
        assert torch.equal(c[:, :N], c_lds[:, :N])
        assert (c[:, N:] == 7.0).all()
        if epi == 1:
            assert torch.equal(b, b_lds)
        assert torch.equal(xd, xr)   # the deep columns written, the others as they were
        want = ref.clamp(min=0) if epi == 1 else ref
        e = ((c[:, :N].double().cpu() - want).abs() / scale).max().item()
        print("gather epi %d M %d N %d K %d: rel err %.3e" % (epi, M, N, K, e))
        assert e < 2e-6
