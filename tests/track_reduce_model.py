"""Lane-level numpy model of the two wave-64 reductions of k_track_pass (gsdf_kernels.hip): wave_sum_to_lane63 (every value
summed in place by six DPP stages, lane 63 ends with the 29 totals) and wave_sum_fold (the values padded to 32; at each stage a
lane pair, quad, octet, row, row pair, half exchanges half of its values, so that lane l < 32 ends with the total of value
bitrev5(l)).  Every instruction of the kernels is one call here, with the operand order of the instruction (src0 + src1), so the
model states which additions are performed on which operand pairs; float32 throughout."""
import numpy as np

LANES = np.arange(64)


def _dpp_src(x, ctrl):
    """(source values, source valid) of a DPP control for x[..., 64]"""
    kind, n = ctrl
    if kind == "row_shr":
        src, valid = LANES - n, (LANES % 16) >= n
    elif kind == "row_shl":
        src, valid = LANES + n, (LANES % 16) + n < 16
    elif kind == "quad_perm":
        src, valid = (LANES & ~3) + np.array(n)[LANES & 3], np.ones(64, bool)
    elif kind == "row_bcast15":
        src, valid = (LANES // 16) * 16 - 1, LANES >= 16
    elif kind == "row_bcast31":
        src, valid = np.full(64, 31), LANES >= 32
    else:
        raise ValueError(kind)
    return x[..., np.where(valid, src, 0)], valid


def add_dpp(old, src0, src1, ctrl, row_mask=0xF, bank_mask=0xF, bound_ctrl=False):
    """v_add_f32_dpp dst, src0, src1: dst = dpp(src0) + src1 in the lanes the masks enable; a lane without a source reads 0
    (bound_ctrl) or is not written; `old` is the previous content of dst"""
    s, valid = _dpp_src(src0, ctrl)
    if bound_ctrl:
        s = np.where(valid, s, np.float32(0))
    en = (((row_mask >> (LANES // 16)) & 1) != 0) & (((bank_mask >> ((LANES % 16) // 4)) & 1) != 0)
    if not bound_ctrl:
        en = en & valid
    with np.errstate(all="ignore"):
        r = (s + src1).astype(np.float32)
    return np.where(en, r, old)


def wave_sum_to_lane63(v):
    """v[..., N, 64] -> the N totals of lane 63"""
    v = v.copy()
    for ctrl, rm, bc in ((("row_shr", 1), 0xF, True), (("row_shr", 2), 0xF, True), (("row_shr", 4), 0xF, True),
                         (("row_shr", 8), 0xF, True), (("row_bcast15", 0), 0xA, False), (("row_bcast31", 0), 0xC, False)):
        for i in range(v.shape[-2]):
            v[..., i, :] = add_dpp(v[..., i, :], v[..., i, :], v[..., i, :], ctrl, row_mask=rm, bound_ctrl=bc)
    return v[..., :, 63]


def _cndmask(a, b, mask):
    """v_cndmask_b32 dst, a, b, mask: b where the lane's mask bit is set"""
    return np.where(((mask >> LANES.astype(np.uint64)) & np.uint64(1)) != 0, b, a)


def _fold_select(w, half, mask, perm):
    """stages 1 and 2: lanes of `mask` keep w[i + half] and send w[i], the others the reverse; the partner is perm's lane"""
    for i in range(half):
        lo, hi = w[..., i, :], w[..., i + half, :]
        send = _cndmask(hi, lo, mask)
        keep = _cndmask(lo, hi, mask)
        w[..., i, :] = add_dpp(keep, send, keep, ("quad_perm", perm))


def _fold_banks(w, half, n, low_banks, high_banks):
    """stages 3 and 4: the low banks take w[i] of the lane n above, the high banks w[i + half] of the lane n below"""
    for i in range(half):
        lo, hi = w[..., i, :], w[..., i + half, :]
        lo = add_dpp(lo, lo, lo, ("row_shl", n), bank_mask=low_banks)
        w[..., i, :] = add_dpp(lo, hi, hi, ("row_shr", n), bank_mask=high_banks)


def permlane16_swap(a, b):
    """v_permlane16_swap_b32 a, b: the odd rows of a change places with the even rows of b"""
    a2, b2 = a.copy(), b.copy()
    for r in (0, 2):
        a2[..., 16 * (r + 1):16 * (r + 2)] = b[..., 16 * r:16 * (r + 1)]
        b2[..., 16 * r:16 * (r + 1)] = a[..., 16 * (r + 1):16 * (r + 2)]
    return a2, b2


def permlane32_swap(a, b):
    """v_permlane32_swap_b32 a, b: lanes 32-63 of a change places with lanes 0-31 of b"""
    a2, b2 = a.copy(), b.copy()
    a2[..., 32:] = b[..., :32]
    b2[..., :32] = a[..., 32:]
    return a2, b2


def bitrev5(l):
    return ((l & 1) << 4) | ((l & 2) << 2) | (l & 4) | ((l & 8) >> 2) | ((l & 16) >> 4)


def wave_sum_fold(v):
    """v[..., N, 64], N <= 32 -> the N totals, gathered from the lanes that hold them (lane l < 32: value bitrev5(l))"""
    n = v.shape[-2]
    w = np.zeros(v.shape[:-2] + (32, 64), np.float32)
    w[..., :n, :] = v
    _fold_select(w, 16, np.uint64(0xAAAAAAAAAAAAAAAA), [1, 0, 3, 2])
    _fold_select(w, 8, np.uint64(0xCCCCCCCCCCCCCCCC), [2, 3, 0, 1])
    _fold_banks(w, 4, 4, 0x5, 0xA)
    _fold_banks(w, 2, 8, 0x3, 0xC)
    with np.errstate(all="ignore"):
        a, b = permlane16_swap(w[..., 0, :], w[..., 1, :])
        s = (a + b).astype(np.float32)                      # rows 0 + 1 and 2 + 3
        a, b = permlane32_swap(s, s.copy())
        t = (a + b).astype(np.float32)                      # (rows 0 + 1) + (rows 2 + 3), in every lane of both halves
    holder = np.array([[l for l in range(32) if bitrev5(l) == i][0] for i in range(n)])
    return t[..., holder]


def same_bits(a, b):
    """equal as float32 words; two NaNs count as equal (which NaN an add of two NaNs returns depends on its operand order, the
    one thing the two trees may differ in)"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
