"""The plan's cls_only_last (csrc/engine.hip: plan; include/lafs_hip.h): host logic with ctx == NULL, one case per rule -- the last
block runs on the cls rows only when the descriptor asks for it AND there is no element dropout AND the weight gradients are not
deferred AND the pass includes block depth - 1.  Everything else of the plan is what it was without the flag."""
import ctypes as C

import test_host_logic as HL


def _plan(_lib, h, d, save, layers=None):
    p = _lib.TrunkPlanInfo()
    rc = h.lafs_trunk_plan(C.byref(d), save, C.byref(p)) if layers is None else h.lafs_trunk_plan_layers(C.byref(d), save, layers[0], layers[1], C.byref(p))
    assert rc == 0, (rc, h.lafs_last_error())
    return p


def test_cls_only_last_one_case_per_rule():
    _lib, h = HL._plan_lib()
    desc = lambda **kw: HL._trunk_desc(_lib, **kw)             # depth 2, two crop groups, 140 sequences
    for save in (0, 1):
        # the flag is opt-in: without it nothing changes, whatever else holds
        assert _plan(_lib, h, desc(), save).cls_only_last == 0
        # set, no dropout, immediate weight gradients, the whole trunk: on
        assert _plan(_lib, h, desc(cls_only_last=1), save).cls_only_last == 1
        # element dropout: a compacted row has lost the absolute row its mask is indexed by
        assert _plan(_lib, h, desc(cls_only_last=1, dropout_p=0.1), save).cls_only_last == 0
        # deferred weight gradients read dense per-layer operand slots
        assert _plan(_lib, h, desc(cls_only_last=1, wgrad_defer=1), save).cls_only_last == 0
        # the pass must include block depth - 1: a backward slice below it is dense, the slice that starts at the top is not
        assert _plan(_lib, h, desc(cls_only_last=1), save, layers=(1, 0)).cls_only_last == 0
        assert _plan(_lib, h, desc(cls_only_last=1), save, layers=(2, 1)).cls_only_last == 1
        assert _plan(_lib, h, desc(cls_only_last=1), save, layers=(2, 0)).cls_only_last == 1
        assert _plan(_lib, h, desc(), save, layers=(2, 0)).cls_only_last == 0
        # the rest of the plan does not depend on the flag
        a, b = _plan(_lib, h, desc(), save), _plan(_lib, h, desc(cls_only_last=1), save)
        assert (a.n_ranges, a.attention, a.mlp_merged) == (b.n_ranges, b.attention, b.mlp_merged)
        assert HL._rp(a.range[0]) == HL._rp(b.range[0]) and HL._rp(a.whole) == HL._rp(b.whole)


def test_plan_layers_refuses_a_bad_range_and_the_workspace_grows_by_the_compact_rows_only():
    _lib, h = HL._plan_lib()
    d = HL._trunk_desc(_lib, cls_only_last=1)
    p = _lib.TrunkPlanInfo()
    for hi, lo in ((3, 0), (1, 1), (0, 0), (2, -1)):
        assert h.lafs_trunk_plan_layers(C.byref(d), 1, hi, lo, C.byref(p)) == -2 and b"bad layer range" in h.lafs_last_error()
    assert h.lafs_trunk_plan_layers(None, 1, 2, 0, C.byref(p)) == -2 and b"null descriptor" in h.lafs_last_error()
    assert h.lafs_trunk_plan_layers(C.byref(d), 1, 2, 0, None) == -2 and b"null plan" in h.lafs_last_error()
    # identity table, two f32 [n_seq, dim] row sets, o_c (bf16 [n_seq, inner]) and lse_c (f32 [n_seq, heads]), each rounded up to 256
    # bytes; when saving also what the last block's two weight-gradient launches (fc2 / fc1 / proj over n_seq rows, qkv over n_tok rows)
    # need beyond the dense block's one launch (csrc/engine.hip: carve).  The default descriptor's workspace is what it was.
    al = lambda n: (n + 255) & ~255
    n_seq, n_tok, D, I, H, M = 140, 9660, 384, 384, 6, 1536
    rows = al(n_seq * 4) + 2 * al(n_seq * D * 4) + al(n_seq * I * 2) + al(n_seq * H * 4)
    it = (_lib.WgradItem * 4)()
    for x, (n1, n2) in zip(it, ((D, M), (M, D), (D, I), (3 * I, D))):     # fc2, fc1, proj, qkv: dW [N1, N2]
        x.N1, x.N2, x.lda, x.ldb, x.ldc = n1, n2, n1, n2, n2
    wg = lambda first, n, m: int(h.lafs_wgrad_group_workspace_bytes(C.cast(C.byref(it[first]), C.POINTER(_lib.WgradItem)), n, m, 0))
    dense = wg(0, 4, n_tok)
    pruned = max(dense, wg(0, 3, n_seq), wg(3, 1, n_tok))
    assert dense > 0 and pruned >= dense
    for save in (0, 1):
        grown = h.lafs_trunk_workspace_bytes(C.byref(d), save) - h.lafs_trunk_workspace_bytes(C.byref(HL._trunk_desc(_lib)), save)
        assert grown == rows + (al(pruned) - al(dense) if save else 0), (save, grown, rows, pruned, dense)
