"""What the GEMM launcher decided before gemm_plan existed, restated in Python from launch_t / launch_partials_t of
kernels/gemm.hip as of the commit before csrc/gemm_plan.cpp: the same if-ladders in the same order, with the
helpers they called (dec_splits_for, dec_plan, launch_dec_w's tile choice, gemm_group_m, launch_reduce_resid_ln,
launch_splitk_reduce). The reference of tests/test_gemm_plan.py.

plan(...) returns the fields of GemmPlan as a dict; a call the launcher refused gives {"error": text}, and
partials(...) (launch_gemm_partials) gives None where the launcher returned 0. Fields a launch did not use are 0
(tiles_n outside the LDS-DMA kernels, gm outside gemm8p_kernel, red_* without a reduce); kc is K when not split.
"""
EPI_STORE, EPI_GELU, EPI_RESID, EPI_GELU_POS, EPI_F32, EPI_CROSSKV, EPI_QKV_DEC, EPI_GELU_F = range(8)
BIG = 256 * 128 * 128


def cdiv(a, b):
    return (a + b - 1) // b


def dec_splits_for(tiles, nk):
    splits = 1
    while tiles * (splits + 1) <= 256 and splits < 12 and (splits + 1) * 2 <= nk:
        splits += 1
    return splits


def dec_plan(N, K, M, ws_elems, dec_splits):
    nk = K // 64
    splits = dec_splits_for(cdiv(N, 64), nk)
    if dec_splits > 0:
        splits = min(dec_splits, nk)
    kc = cdiv(nk, splits) * 64
    splits = cdiv(K, kc)
    if splits * M * N > ws_elems:
        return 0, 0
    return splits, kc


def _launch(kernel, bm, bn, grid, threads, split, splits, kc, tiles_n=0, gm=0):
    gx, gy, gz = grid
    return dict(kernel=kernel, bm=bm, bn=bn, grid_x=gx, grid_y=gy, grid_z=gz, threads=threads, tiles_n=tiles_n,
                split=int(split), splits=splits, kc=kc, gm=gm, reduce="none", red_grid=0, red_threads=0, red_npt=0)


def _launch_dec(M, N, tiles, splits, kc, split, dec_bm):
    if M <= 32 and dec_bm <= 32:
        return _launch("dec", 32, 64, (tiles, 1, splits), 256, split, splits, kc)
    if M <= 64 and dec_bm <= 64:
        return _launch("dec", 64, 64, (tiles, 1, splits), 256, split, splits, kc)
    return _launch("dec", 128, 64, (tiles, cdiv(M, 128), splits), 256, split, splits, kc)


def _reduce_resid_ln(p, M, N, splits, ln4=True):
    if ln4 and N % 4 == 0 and N <= 4096 and splits <= 16:
        p.update(reduce="ln4", red_grid=M, red_threads=cdiv(N // 4, 64) * 64)
        return p
    npt = cdiv(N, 256)
    if npt <= 4:
        p.update(reduce="ln", red_grid=M, red_threads=256, red_npt=4)
    elif npt <= 8:
        p.update(reduce="ln", red_grid=M, red_threads=256, red_npt=8)
    else:
        return {"error": "fused LN width %d > 2048" % N}
    return p


def _splitk_reduce(p, M, N):
    total = M * N
    work = total // 4 if N % 4 == 0 else total
    thr = 64 if work < 65536 else 256
    p.update(reduce="plain", red_grid=min(4096, cdiv(work, thr)), red_threads=thr)
    return p


def plan(epi, M, N, K, has_ws, ws_elems, fused_ln, w8, variant=-1, dec_splits=0, dec_bm=32, gm_env=-1):
    """launch_t<T, epi> of a GemmArgs with these M, N, K, splitk_ws (has_ws) / splitk_ws_elems, ln_out (fused_ln is
    EPI_RESID with ln_out set) and w8_scale (w8)."""
    assert not fused_ln or epi == EPI_RESID
    if w8:
        if not (has_ws and M <= 128 and K % 64 == 0 and variant != 0 and (epi != EPI_RESID or fused_ln)):
            return {"error": "e4m3 weights need the decode-step GEMM path (M %d <= 128, K %% 64 == 0)" % M}
    big256 = variant >= 2 or (variant < 0 and (N % 256 == 0 or N >= 1024) and M >= 1024)
    if M * N >= BIG and K % 64 == 0 and big256:
        tn = cdiv(N, 256)
        gm = gm_env if gm_env >= 0 else (4 if tn >= 8 else 0)
        return _launch("8p", 256, 256, (tn * cdiv(M, 256), 1, 1), 512, False, 1, K, tiles_n=tn, gm=gm)
    if M * N >= BIG and K % 64 == 0 and variant != 0:
        tn = cdiv(N, 128)
        return _launch("glds", 128, 128, (tn * cdiv(M, 128), 1, 1), 256, False, 1, K, tiles_n=tn)
    if M * N >= BIG:
        return _launch("reg", 128, 128, (cdiv(N, 128), cdiv(M, 128), 1), 256, False, 1, K)
    nk = cdiv(K, 64)
    if has_ws and (M <= 128 or not fused_ln) and K % 64 == 0 and variant != 0:
        tiles = cdiv(N, 64)
        splits, kc = dec_plan(N, K, M, ws_elems, dec_splits)
        small_unsplit = splits == 1 and not fused_ln and M <= 64 and not w8
        if w8 and not splits:
            return {"error": "e4m3 decode GEMM: split-K workspace too small"}
        if splits and not small_unsplit:
            if splits == 1 and not fused_ln:
                return _launch_dec(M, N, tiles, 1, kc, False, dec_bm)
            p = _launch_dec(M, N, tiles, splits, kc, True, dec_bm)
            if fused_ln:
                return _reduce_resid_ln(p, M, N, splits)
            return _splitk_reduce(p, M, N)
    if has_ws and M <= 128:
        BM = 64 if M <= 64 else 128
        tiles = cdiv(N, 64)
        splits = min(max(1, 128 // tiles), max(1, nk // 4))
        while splits > 1 and splits * M * N > ws_elems:
            splits -= 1
        if splits > 1 or fused_ln:
            kc = cdiv(cdiv(K, splits), 64) * 64
            splits = cdiv(K, kc)
            p = _launch("reg", BM, 64, (tiles, 1, splits), 256, True, splits, kc)
            if fused_ln:
                return _reduce_resid_ln(p, M, N, splits, False)
            return _splitk_reduce(p, M, N)
        return _launch("reg", BM, 64, (tiles, 1, 1), 256, False, 1, K)
    if fused_ln:
        return {"error": "fused LN requires the decode split-K path"}
    tiles = cdiv(N, 64) * cdiv(M, 64)
    splits = min(16, max(1, 512 // tiles))
    splits = min(splits, max(1, nk // 2))
    while splits > 1 and splits * M * N > ws_elems:
        splits -= 1
    if not has_ws or splits <= 1:
        return _launch("reg", 64, 64, (cdiv(N, 64), cdiv(M, 64), 1), 256, False, 1, K)
    kc = cdiv(cdiv(K, splits), 64) * 64
    splits = cdiv(K, kc)
    p = _launch("reg", 64, 64, (cdiv(N, 64), cdiv(M, 64), splits), 256, True, splits, kc)
    p.update(reduce="plain", red_grid=min(1024, cdiv(M * N, 256)), red_threads=256)
    return p


def partials(M, N, K, has_ws, ws_elems, dec_splits=0, dec_bm=32):
    """launch_partials_t: the split form of gemm_dec_kernel whatever the split count, no reduce; None = it returned 0."""
    if not has_ws or M > 128 or K % 64 != 0:
        return None
    splits, kc = dec_plan(N, K, M, ws_elems, dec_splits)
    if not splits:
        return None
    return _launch_dec(M, N, cdiv(N, 64), splits, kc, True, dec_bm)


FIELDS = ("kernel", "bm", "bn", "grid_x", "grid_y", "grid_z", "threads", "tiles_n", "split", "splits", "kc", "gm", "reduce",
          "red_grid", "red_threads", "red_npt")


def line(p):
    """A plan as tools/gemm_plan_check.cpp prints it."""
    if p is None:
        return "none"
    if "error" in p:
        return "error " + p["error"]
    return " ".join(str(p[f]) for f in FIELDS)
