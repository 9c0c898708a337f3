"""The K-resident GEMM's partition (csrc/gemm_kres.hip: kres_partition): a workgroup gets a contiguous part of ONE 128-row unit's
64-column blocks and loads its resident rows once -- or, where such parts would leave too many workgroup slots empty, an equal run
of the unit-major item list that may reach into a second unit.

GPU: every epilogue form the route accepts, at row counts whose last unit is full / holds one live row (three idle waves) / is
ragged, and at N = 64 (one block per unit: one part), 384, 1152 and 1536, against the fp64 oracle of tests/fp64_bounds.py through
the very harness of tests/test_gpu_gemm.py (`run`: route 1 asserted through lafs_gemm_nt_route, NaN-filled outputs with guard rows
past M and guard columns that must stay bit-identical, every owned element overwritten and within its bound).  The pre-training
step's own launches -- two and three parts per unit at 197 and 148 units, equal runs for N = 1152 at 197 units and for 345 units --
fewer workgroup slots (LAFS_OPT_COMM_CUS) and more units than slots are cases of their own.

Host: what lafs_gemm_nt_plan reports for a sweep of shapes, and that the partition the kernel derives from (grid, parts) covers
every (unit, block) exactly once; with parts, no workgroup's items lie in two units."""
import ctypes as C

import pytest

import gemm_cases as gc

SLOTS = 512                              # two 4-wave workgroups on each of 256 CUs
OPT_COMM_CUS = 6                         # LAFS_OPT_COMM_CUS
FORMS = gc.FORMS[:5] + gc.FORMS[6:8]     # bf16, gelu_u, gelu_noC, gelu_save, resid (seq_scale / row2seq), dgelu_u, dgelu_save
ROWS = (2048, 2049, 2048 + 97, 128 * 37 + 5)
COLS = (64, 384, 1152, 1536)


def _cases():
    g = [gc.nt_case(f"kres-M{M}-N{N}-{tag}", epi, M, N, 384, route=1, **o) for M in ROWS for N in COLS for tag, epi, o in FORMS]
    # the step's launches.  197 units x 2 parts of 3 blocks: the projection forward (fp32 residual) and its input gradient on the
    # long row chain; 148 units x 3 parts of 6 blocks: qkv on the short one; equal runs: qkv on the long chain (2 parts would be
    # 9 items against runs of 6.9) and the merged chains' 345 units (one part per unit would fill 352 of 512 slots)
    g.append(gc.nt_case("kres-step-M25216-N384-resid", gc.EPI_RESID_F32, 25216, 384, 384, route=1))
    g.append(gc.nt_case("kres-step-M25216-N384-bf16", gc.EPI_BF16, 25216, 384, 384, route=1))
    g.append(gc.nt_case("kres-step-M18944-N1152-bf16", gc.EPI_BF16, 18944, 1152, 384, route=1))
    g.append(gc.nt_case("kres-step-M25216-N1152-bf16-runs", gc.EPI_BF16, 25216, 1152, 384, route=1))
    g.append(gc.nt_case("kres-step-M44160-N384-resid-runs", gc.EPI_RESID_F32, 44160, 384, 384, route=1))
    # 64 CUs left to the collectives: 384 slots, 38 units x 10 parts of 2-3 blocks
    g.append(gc.nt_case("kres-comm64-M4741-N1536-gelu_save", gc.EPI_BF16_GELU, 128 * 37 + 5, 1536, 384, route=1, form="save",
                        opts={OPT_COMM_CUS: 64}))
    # 192 CUs left: 128 slots for 131 units -- equal runs of 3.07 items, most of them over two units (a second row load)
    for tag, epi, o in (gc.FORMS[4], gc.FORMS[1], gc.FORMS[6]):
        g.append(gc.nt_case(f"kres-comm192-M16645-N192-{tag}", epi, 128 * 130 + 5, 192, 384, route=1, opts={OPT_COMM_CUS: 192}, **o))
    return g


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_kres_parts_against_fp64(c):
    from test_gpu_gemm import run
    assert run(c), c["id"]


# ------------------------------------------------------------------------------------------------ host: the plan and the partition
def expected_grid(units, cbn, slots=SLOTS):
    """(parts, workgroups).  parts = the largest p <= cbn with units * p <= slots, the grid rounded up to the 8 XCDs -- unless such a
    part, ceil(cbn / p) items, is more than 1.5 items (the worth of a row load) longer than an equal run over all slots, or there are
    more units than slots: then (0, slots), equal runs."""
    p = min(cbn, slots // units)
    if p < 1 or -(-cbn // p) > units * cbn / slots + 1.5:
        return 0, slots
    return p, (units * p + 7) // 8 * 8


def parts_of(grid, parts, units, cbn):
    """[first item, end item) of the unit-major item list per logical workgroup id, as gemm_kres_kernel derives them."""
    out = []
    for wid in range(grid):
        if parts > 0:
            part, mu = wid % parts, wid // parts
            if mu < units:
                out.append((mu * cbn + cbn * part // parts, mu * cbn + cbn * (part + 1) // parts))
        else:
            out.append((units * cbn * wid // grid, units * cbn * (wid + 1) // grid))
    return out


def test_plan_grid_and_partition_cover_every_item_once():
    import os
    from lafs_cvpr2024_amd import _lib
    assert os.path.isfile(_lib.LIB_PATH), "library not built"
    h = _lib.lib()
    rows = (2048, 2049, 2145, 4741, 16645, 18944, 25216, 44160, 65536, 65537, 70000, 131072, 200001)
    for M in rows:
        for N in range(64, 1537, 64):
            a = _lib.GemmNTArgs()
            a.M, a.N, a.K, a.epilogue, a.splits = M, N, 384, _lib.EPI_BF16, 1
            a.lda, a.ldb, a.ldc = 384, 384, N
            a.A = a.B = a.C = 1 << 20                      # (never dereferenced: the plan reads shapes, strides and presence)
            info = _lib.GemmNTPlanInfo()
            assert int(h.lafs_gemm_nt_plan(C.byref(a), C.byref(info))) == 0 and info.route == 1, (M, N)
            units, cbn, G = (M + 127) // 128, N // 64, info.workgroups
            assert G <= SLOTS and G % 8 == 0 and G > 0, (M, N, G)
            if units <= SLOTS:
                assert G >= units, (M, N, G)
            parts, grid = expected_grid(units, cbn)
            assert G == grid, (M, N, G, grid)
            seen = [0] * (units * cbn)
            sizes = set()
            for ib, ie in parts_of(G, parts, units, cbn):
                assert 0 <= ib < ie <= units * cbn, (M, N, ib, ie)
                if parts > 0:                               # a part stays inside one unit
                    assert ib // cbn == (ie - 1) // cbn, (M, N, ib, ie)
                sizes.add(ie - ib)
                for i in range(ib, ie):
                    seen[i] += 1
            assert all(v == 1 for v in seen), (M, N)
            assert max(sizes) - min(sizes) <= 1, (M, N, sizes)
    # the shapes of the pre-training step: N = 384 and N = 1152 on 197 / 148 / 345 units
    assert [expected_grid(u, 6) for u in (197, 148, 345)] == [(2, 400), (3, 448), (0, 512)]
    assert [expected_grid(u, 18) for u in (197, 148, 345)] == [(0, 512), (3, 448), (0, 512)]
