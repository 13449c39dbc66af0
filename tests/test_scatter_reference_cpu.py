"""CPU: the float64 table-gradient scatter of the oracle (orc.hashgrid_scatter64), which the GPU scatter tests
(tests/test_gpu_table_scatter.py) hold the kernels to entry by entry, pinned to torch autograd through the oracle's own
hash encoding: bit for bit with a float64 table, to fp32 rounding with an fp32 one."""
import numpy as np
import pytest
import torch

from oracle import nerfacto_oracle as orc


def _points(M, min_res, seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0, 1, (M, 3)).astype(np.float32)
    x[:64] = np.round(x[:64] * min_res) / min_res  # on lattice planes of the coarsest level (ceil == floor there)
    x[64:96] = rs.randint(0, 2, (32, 3))           # the box's corners
    x[96:128, 0] = 1.0
    x[128:160] = x[0:32]                           # repeated points: several contributions per entry
    g = rs.standard_normal((M, 2)) * 10.0 ** rs.uniform(-8, 0, (M, 2))
    return torch.from_numpy(x), g


@pytest.mark.parametrize("L,min_res,max_res,log2_T", [(5, 16, 128, 10), (16, 16, 2048, 12), (1, 4, 4, 6)])
def test_scatter64_is_autograd_of_the_oracle_encoding(L, min_res, max_res, log2_T):
    M, T = 3001, 1 << log2_T
    x, _ = _points(M, min_res, L)
    rs = np.random.RandomState(L + 1)
    denc = torch.from_numpy((rs.standard_normal((M, 2 * L)) * 10.0 ** rs.uniform(-8, 0, (M, 2 * L))).astype(np.float32))
    denc[rs.uniform(0, 1, M) < 0.2] = 0.0
    scal = orc.hash_level_scalings(L, min_res, max_res)
    ref, ab, cnt = orc.hashgrid_scatter64(x, denc, scal, T)
    assert ref.dtype == ab.dtype == cnt.dtype == torch.float64 and ref.shape == (L * T, 2)
    assert int(cnt.sum()) == 16 * M * L  # 8 corners x 2 features per point and level, coinciding corners counted twice
    assert bool((ab * (1 + 1e-12) >= ref.abs()).all()) and bool(((cnt == 0) <= (ab == 0)).all())
    # float64 table leaf: autograd's accumulation, bit for bit
    t64 = torch.zeros(L * T, 2, dtype=torch.float64, requires_grad=True)
    (orc.hashgrid_encode(x, t64, scal, T) * denc.double()).sum().backward()
    assert torch.equal(t64.grad, ref)
    # fp32 table: each contribution three fp32 products, the sum in fp32 (n_e - 1 additions)
    t32 = torch.zeros(L * T, 2, requires_grad=True)
    (orc.hashgrid_encode(x, t32, scal, T) * denc).sum().backward()
    err = (t32.grad.double() - ref).abs()
    assert bool((err <= (cnt + 3) * 2.0**-24 * ab + cnt * 2.0**-126).all())
    assert float(err.max()) > 0  # (the fp32 evaluation does round: the comparison above is not vacuous)
    # counts: every contribution of a point on a lattice plane lands on an entry twice
    x1 = x[64:65]  # a box corner: every level's cell collapses to one lattice point, 8 contributions on one entry
    _, _, c1 = orc.hashgrid_scatter64(x1, torch.ones(1, 2 * L), scal, T)
    assert sorted(set(c1[c1 != 0].tolist())) == [8.0] and int((c1 != 0).sum()) == 2 * L
