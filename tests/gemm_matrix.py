"""Route table of the GEMM family (openp5_amd/csrc/p5_gemm_tu.hip: launch_gemm_impl, launch_gemm_tile, launch_gemm4; the decode step's
p5_op_skinny_gemm in p5_lib.hip): one entry per launch route, each at the edges of its conditions, with the launch site it must reach.
Shared by the emulator and the GPU tests of cases.gemm_ref_case; tests/test_static.py checks that every GEMM launch site of
p5_gemm_tu.hip is named here.

A row is a dict:
  id        test id
  op        "gemm" (p5_op_gemm; dtype 0 fp32, 1 bf16, 2 fp32 operands with split-f16 products), "group" (p5_op_gemm_group, `cfg` = tile_cfg,
            `ks`, `probs`), "skinny" (p5_op_skinny_gemm, `amode`)
  M N K a_ks b_ks epi c_f32 splitk
  pad       extra elements of (lda, ldb, ldc, ldaux) beyond the least legal leading dimension (see cases.gemm_ref_case)
  alpha     epilogue scale (default 0.75 on epilogues 0, 3, 4, 6, else 1)
  drop      dropout probability (default 0.1 on epilogues 1, 2)
  opts      p5_set_option values the row needs (restored afterwards)
  site      the P5_LAUNCH kernel text of the route (whitespace-insensitive); tag: the P5_PROF_TAG the in-run profiler reports with it
            ("" = the site sets none; None = not checked, the skinny kernels)
  gpu_only  too large for the emulator
  checked_by  launch sites whose epilogues have dedicated tests elsewhere (no cases.gemm_ref_case run)
"""

# launch sites (P5_LAUNCH first arguments in p5_gemm_tu.hip)
S_G3 = "p5_gemm3_kernel<BM, BN, 2, 4>"
S_RING4 = "p5_gemm2_kernel<BM, BN, 4>"
S_V2_3 = "p5_gemm2_kernel<BM, BN, 3>"
S_V2_2 = "p5_gemm2_kernel<BM, BN, 2>"
S_WG3 = "p5_gemm2_kernel<BM, BN, 3, true, true>"
S_WG4 = "p5_gemm2_kernel<BM, BN, 4, true, true>"
S_SR0 = "p5_gemm2_kernel<BM, BN, 8, false, false>"
S_SR1 = "p5_gemm2_kernel<BM, BN, 8, false, true>"
S_SR3 = "p5_gemm2_kernel<BM, BN, 8, true, true>"
S_R32 = "p5_gemm2_kernel<32, 64, 8, false, false>"
S_SPLIT = "p5_gemm_split_kernel<BM, BN>"
S_SPLIT_FB = "p5_gemm_kernel<T, BM, BN, false, false, 2, false, false, 1>"
S_KC_DMA = "p5_gemm_kernel<T, BM, BN, false, false, 2, sizeof(T) == 2, sizeof(T) == 2>"
S_KC = "p5_gemm_kernel<T, BM, BN, false, false, 2, false, false>"
S_M1_KSDMA = "p5_gemm_kernel<T, BM, BN, false, true, 2, sizeof(T) == 2, sizeof(T) == 2>"
S_M3_KSDMA = "p5_gemm_kernel<T, BM, BN, true, true, 2, sizeof(T) == 2, sizeof(T) == 2>"
S_M1_DMA = "p5_gemm_kernel<T, BM, BN, false, true, 2, sizeof(T) == 2, false>"
S_M1 = "p5_gemm_kernel<T, BM, BN, false, true, 2, false, false>"
S_M3 = "p5_gemm_kernel<T, BM, BN, true, true, 2, false, false>"
S_G4 = "p5_gemm4_kernel<BM, BN, WMW, WNW, NST, KS, 0, OCC>"
S_G5 = "p5_gemm5_kernel<false>"
S_G5_KS = "p5_gemm5_kernel<true>"
S_G5_128 = "p5_gemm5_kernel<false, 0, 0, 128>"
S_G5_NBW = "p5_gemm5_kernel<false, 0, 3, 128>"
S_G5_CE = "p5_gemm5_kernel<false, 0, 2>"
S_G5_GATE = "p5_gemm5_kernel<false, 0, 1>"

T_WIDE = "KC: forward / data-gradient GEMMs"
T_WS128 = "KC 128x128: N = d_model outputs"
T_G5KS = "KS: grouped weight gradients"

# options that let the emulator reach a route at small sizes (the GPU rows of the same route run the same shapes under them)
LOW_WIDE = {"gemm_wide_min_tiles": 1}
LOW_WS128 = {"gemm_wide_min_tiles": 100000, "gemm_ring128_min_tiles": 1, "gemm_ws128_min_k": 64}
LOW_N512 = {"gemm_wide_min_tiles": 100000, "gemm_ws128": 0, "gemm_ring128_min_tiles": 1, "gemm_ring128_min_k": 64}


def _row(id, site, tag, op="gemm", dtype=1, M=1, N=1, K=64, a_ks=0, b_ks=0, epi=0, c_f32=0, splitk=1, pad=(0, 0, 8, 16), alpha=None,
         drop=None, opts=None, **kw):
    r = dict(id=id, op=op, dtype=dtype, M=M, N=N, K=K, a_ks=a_ks, b_ks=b_ks, epi=epi, c_f32=c_f32, splitk=splitk, pad=pad,
             alpha=(0.75 if epi in (0, 3, 4, 6) else 1.0) if alpha is None else alpha, drop=(0.1 if epi in (1, 2) else 0.0) if drop is None else drop,
             opts=dict(opts or {}), site=site, tag=tag, gpu_only=False, checked_by=None)
    r.update(kw)
    return r


def _gemm_rows():
    R = []
    # ---- bf16, wide 256x128 persistent ring (p5_gemm5_kernel<false>; gemm_ws 0: p5_gemm4_kernel 256x128) -------------------------------
    for M, N, K, epi, pad in [(256, 128, 64, 0, (0, 0, 8, 16)), (257, 129, 128, 1, (64, 0, 0, 16)), (1, 136, 64, 2, (0, 64, 8, 8)),
                              (300, 1, 192, 3, (0, 0, 8, 16)), (512, 256, 128, 2, (0, 0, 0, 8))]:
        R.append(_row(f"wide-{M}x{N}x{K}-e{epi}", S_G5, T_WIDE, M=M, N=N, K=K, epi=epi, pad=pad, opts=LOW_WIDE))
    for M, N, K, epi in [(256, 128, 64, 0), (257, 200, 128, 1), (130, 72, 64, 3)]:
        R.append(_row(f"wide-ws0-{M}x{N}x{K}-e{epi}", S_G4, "256x128 KC", M=M, N=N, K=K, epi=epi, opts=dict(LOW_WIDE, gemm_ws=0)))
    # ---- bf16, ws128: p5_gemm5_kernel<false, 0, 0, 128> (N = d_model outputs) -----------------------------------------------------
    for M, N, K, epi, pad in [(128, 128, 64, 0, (0, 0, 8, 16)), (129, 129, 128, 2, (64, 0, 8, 16)), (1, 64, 64, 1, (0, 0, 0, 8)),
                              (200, 1, 128, 3, (0, 64, 8, 16))]:
        R.append(_row(f"ws128-{M}x{N}x{K}-e{epi}", S_G5_128, T_WS128, M=M, N=N, K=K, epi=epi, pad=pad, opts=LOW_WS128))
    # ---- bf16, ring n512: p5_gemm2_kernel<128, 128, 4> ------------------------------------------------------------------------------
    for M, N, K, epi, pad in [(128, 128, 64, 0, (0, 0, 8, 16)), (129, 129, 128, 1, (64, 64, 8, 16)), (1, 40, 64, 2, (0, 0, 0, 8)),
                              (150, 1, 192, 3, (0, 0, 8, 16)), (130, 136, 128, 6, (0, 0, 8, 16))]:
        R.append(_row(f"n512-{M}x{N}x{K}-e{epi}", S_RING4, "bf16 128x128 KC", M=M, N=N, K=K, epi=epi, c_f32=int(epi == 6), pad=pad, opts=LOW_N512))
    # ---- bf16, weight-gradient ring (both KS, epilogue 4): automatic split-K at default options (GPU), forced instances (emulator) ----
    R.append(_row("wgrad-ring4-auto-768x1024x2048", S_WG4, "bf16 128x128 KS", M=768, N=1024, K=2048, a_ks=1, b_ks=1, epi=4, c_f32=1,
                  splitk=0, gpu_only=True))
    R.append(_row("wgrad-ring3-auto-1024x768x4096", S_WG3, "bf16 128x128 KS", M=1024, N=768, K=4096, a_ks=1, b_ks=1, epi=4, c_f32=1,
                  splitk=0, opts={"gemm_v2": 3}, gpu_only=True))
    for st, site in ((4, S_WG4), (3, S_WG3)):
        for M, N, K, sk in [(128, 128, 64, 1), (129, 136, 256, 2), (1, 72, 128, 1), (200, 8, 192, 3)]:
            R.append(_row(f"wgrad-ring{st}-{M}x{N}x{K}-s{sk}", site, "bf16 128x128 KS", M=M, N=N, K=K, a_ks=1, b_ks=1, epi=4, c_f32=1, splitk=sk,
                          opts={"gemm_tile": 128, "gemm_v2": st}))
    # ---- bf16, 8-slot small ring (64x64) in modes 0, 1, 3 ----------------------------------------------------------------------------
    for M, N, K, epi in [(64, 64, 256, 0), (65, 72, 320, 2), (1, 64, 256, 1), (130, 1, 256, 3)]:
        R.append(_row(f"ring8-m0-{M}x{N}x{K}-e{epi}", S_SR0, "bf16 64x64 KC", M=M, N=N, K=K, epi=epi, opts={"gemm_ring32": 0}))
    for M, N, K, epi in [(64, 64, 256, 0), (65, 72, 320, 2), (1, 8, 256, 3)]:
        R.append(_row(f"ring8-m1-{M}x{N}x{K}-e{epi}", S_SR1, "bf16 64x64 KC/KS", M=M, N=N, K=K, b_ks=1, epi=epi))
    for M, N, K, epi, c in [(64, 64, 256, 4, 1), (72, 65, 1024, 4, 1), (8, 1, 256, 0, 0), (70, 130, 256, 6, 1)]:
        R.append(_row(f"ring8-m3-{M}x{N}x{K}-e{epi}", S_SR3, "bf16 64x64 KS", M=M, N=N, K=K, a_ks=1, b_ks=1, epi=epi, c_f32=c))
    # ---- bf16, 32x64 ring ----------------------------------------------------------------------------------------------------------
    for M, N, K, epi, pad in [(32, 64, 256, 0, (0, 0, 8, 16)), (33, 65, 320, 2, (8, 16, 8, 24)), (1, 1, 256, 1, (0, 0, 0, 8)),
                              (512, 128, 256, 3, (0, 0, 8, 16))]:
        R.append(_row(f"ring32-{M}x{N}x{K}-e{epi}", S_R32, "", M=M, N=N, K=K, epi=epi, pad=pad))
    # ---- bf16, 256x256 (p5_gemm3_kernel): forced, through lda % 64 != 0, through epilogue 4 / 6 and gemm_wide 0 at default thresholds ----
    for M, N, K, epi, c, pad in [(256, 256, 64, 0, 0, (0, 0, 8, 16)), (257, 257, 128, 2, 0, (8, 0, 8, 16)), (1, 200, 64, 4, 1, (0, 0, 8, 8)),
                                 (300, 1, 128, 6, 1, (0, 0, 0, 8)), (100, 130, 64, 1, 0, (0, 8, 8, 16))]:
        R.append(_row(f"g3-forced-{M}x{N}x{K}-e{epi}", S_G3, "bf16 256x256", M=M, N=N, K=K, epi=epi, c_f32=c, pad=pad, opts={"gemm_tile": 256}))
    R.append(_row("g3-auto-lda-4096x4096x1024", S_G3, "bf16 256x256", M=4096, N=4096, K=1024, pad=(8, 0, 8, 16), gpu_only=True))
    R.append(_row("g3-auto-accum-4096x4096x1024", S_G3, "bf16 256x256", M=4096, N=4096, K=1024, epi=6, c_f32=1, gpu_only=True))
    R.append(_row("g3-auto-wide0-4097x4096x1024", S_G3, "bf16 256x256", M=4097, N=4096, K=1024, epi=2, opts={"gemm_wide": 0}, gpu_only=True))
    # ---- bf16 p5_gemm_kernel, 64x64 and 128x128, every mode / DMA / KS-DMA branch --------------------------------------------------
    for tile, small in ((64, {"gemm_small_ring": 0}), (128, {"gemm_tile": 128})):
        sz = (tile, tile)
        tg = f"bf16 {tile}x{tile}"
        R += [
            _row(f"t{tile}-kc-dma-{sz[0]}x{sz[1]}x64-e0", S_KC_DMA, f"{tg} KC", M=sz[0], N=sz[1], K=64, opts=small),
            _row(f"t{tile}-kc-dma-{sz[0] + 1}x{sz[1] + 1}x128-e2", S_KC_DMA, f"{tg} KC", M=sz[0] + 1, N=sz[1] + 1, K=128, epi=2, pad=(64, 8, 8, 16), opts=small),
            _row(f"t{tile}-kc-dma-1x{sz[1]}x192-e1", S_KC_DMA, f"{tg} KC", M=1, N=sz[1], K=192, epi=1, opts=small),
            _row(f"t{tile}-kc-72x1x64-e3", S_KC_DMA, f"{tg} KC", M=72, N=1, K=64, epi=3, opts=small),
            _row(f"t{tile}-kc-k40-{sz[0]}x{sz[1]}x40-e0", S_KC, f"{tg} KC", M=sz[0], N=sz[1], K=40, opts=small),
            _row(f"t{tile}-kc-k104-{sz[0] + 1}x{sz[1] + 3}x104-e2", S_KC, f"{tg} KC", M=sz[0] + 1, N=sz[1] + 3, K=104, epi=2, pad=(8, 16, 8, 8), opts=small),
            _row(f"t{tile}-kc-k8-1x16x8-e1", S_KC, f"{tg} KC", M=1, N=16, K=8, epi=1, opts=small),
            _row(f"t{tile}-ktail-70x40x50", S_KC, f"{tg} KC", M=70, N=40, K=50, pad=(0, 8, 8, 16), opts=small),
            _row(f"t{tile}-ktail-65x33x3-e3", S_KC, f"{tg} KC", M=65, N=33, K=3, epi=3, opts=small),
            _row(f"t{tile}-m1-ksdma-{sz[0]}x{sz[1]}x64-e0", S_M1_KSDMA, f"{tg} KC" if tile == 128 else f"{tg} KC/KS", M=sz[0], N=sz[1], K=64, b_ks=1, opts=small),
            _row(f"t{tile}-m1-ksdma-{sz[0] + 1}x{sz[1] + 1}x128-e3", S_M1_KSDMA, f"{tg} KC" if tile == 128 else f"{tg} KC/KS", M=sz[0] + 1, N=sz[1] + 1,
                 K=128, b_ks=1, epi=3, pad=(64, 8, 8, 16), opts=small),
            _row(f"t{tile}-m3-ksdma-{sz[0]}x{sz[1]}x64-e4", S_M3_KSDMA, f"{tg} KS", M=sz[0], N=sz[1], K=64, a_ks=1, b_ks=1, epi=4, c_f32=1, opts=small),
            _row(f"t{tile}-m3-ksdma-{sz[0] + 1}x1x192-e4-s2", S_M3_KSDMA, f"{tg} KS", M=sz[0] + 1, N=1, K=192, a_ks=1, b_ks=1, epi=4, c_f32=1, splitk=2,
                 pad=(8, 8, 8, 8), opts=small),
            _row(f"t{tile}-m3-ksdma-1x{sz[1] + 1}x128-e0", S_M3_KSDMA, f"{tg} KS", M=1, N=sz[1] + 1, K=128, a_ks=1, b_ks=1, epi=0, opts=small),
            _row(f"t{tile}-m1-ksdma0-{sz[0] + 1}x{sz[1]}x64-e2", S_M1_DMA, f"{tg} KC" if tile == 128 else f"{tg} KC/KS", M=sz[0] + 1, N=sz[1], K=64,
                 b_ks=1, epi=2, opts=dict(small, gemm_ksdma=0)),
            _row(f"t{tile}-m3-ksdma0-{sz[0]}x{sz[1] + 1}x128-e6", S_M3, f"{tg} KS", M=sz[0], N=sz[1] + 1, K=128, a_ks=1, b_ks=1, epi=6, c_f32=1,
                 opts=dict(small, gemm_ksdma=0)),
            _row(f"t{tile}-m1-k40-{sz[0] + 1}x{sz[1] + 1}x40-e0", S_M1, f"{tg} KC" if tile == 128 else f"{tg} KC/KS", M=sz[0] + 1, N=sz[1] + 1, K=40,
                 b_ks=1, opts=small),
            _row(f"t{tile}-m3-k40-{sz[0] + 1}x{sz[1] + 1}x40-e4", S_M3, f"{tg} KS", M=sz[0] + 1, N=sz[1] + 1, K=40, a_ks=1, b_ks=1, epi=4, c_f32=1,
                 opts=small),
        ]
    R.append(_row("t128-auto-2048x4096x64", S_KC_DMA, "bf16 128x128 KC", M=2048, N=4096, K=64, epi=1, opts={"gemm_wide": 0}, gpu_only=True))
    # ---- gemm_v2 2- and 3-stage kernels (forced 128x128 tiles) -----------------------------------------------------------------------
    for st, site in ((2, S_V2_2), (3, S_V2_3)):
        for M, N, K, epi in [(128, 128, 64, 0), (129, 136, 192, 2), (1, 1, 128, 1), (200, 72, 256, 3)]:
            R.append(_row(f"v2s{st}-{M}x{N}x{K}-e{epi}", site, "bf16 128x128 KC", M=M, N=N, K=K, epi=epi, opts={"gemm_tile": 128, "gemm_v2": st}))
    # ---- bf16 automatic split-K for epilogue 4 (p5_gemm_kernel, K above the small ring's 1024) ---------------------------------------
    R.append(_row("autosplit-m3-64x72x2048-e4", S_M3_KSDMA, "bf16 64x64 KS", M=64, N=72, K=2048, a_ks=1, b_ks=1, epi=4, c_f32=1, splitk=0))
    R.append(_row("autosplit-m1-65x8x1152-e4", S_M1_KSDMA, "bf16 64x64 KC/KS", M=65, N=8, K=1152, b_ks=1, epi=4, c_f32=1, splitk=0))
    R.append(_row("autosplit-kc-1x64x1088-e4", S_KC_DMA, "bf16 64x64 KC", M=1, N=64, K=1088, epi=4, c_f32=1, splitk=0))
    # ---- fp32 operands: 64x64 and 128x128 p5_gemm_kernel ----------------------------------------------------------------------------
    for tile, opts in ((64, {}), (128, {"gemm_tile": 128})):
        tg = f"f32 {tile}x{tile}"
        R += [
            _row(f"f32-t{tile}-kc-{tile}x{tile}x32-e0", S_KC, tg, dtype=0, M=tile, N=tile, K=32, opts=opts),
            _row(f"f32-t{tile}-kc-{tile + 1}x{tile + 1}x72-e2", S_KC, tg, dtype=0, M=tile + 1, N=tile + 1, K=72, epi=2, pad=(4, 8, 8, 4), opts=opts),
            _row(f"f32-t{tile}-kc-1x3x4-e1", S_KC, tg, dtype=0, M=1, N=3, K=4, epi=1, opts=opts),
            _row(f"f32-t{tile}-ktail-70x40x50-e0", S_KC, tg, dtype=0, M=70, N=40, K=50, opts=opts),
            _row(f"f32-t{tile}-ktail-9x130x7-e3", S_KC, tg, dtype=0, M=9, N=130, K=7, epi=3, opts=opts),
            _row(f"f32-t{tile}-m1-{tile + 1}x{tile}x48-e0", S_M1, tg, dtype=0, M=tile + 1, N=tile, K=48, b_ks=1, opts=opts),
            _row(f"f32-t{tile}-m3-{tile}x{tile + 1}x40-e4", S_M3, tg, dtype=0, M=tile, N=tile + 1, K=40, a_ks=1, b_ks=1, epi=4, c_f32=1, opts=opts),
            _row(f"f32-t{tile}-m3-{tile + 1}x1x96-e4-s3", S_M3, tg, dtype=0, M=tile + 1, N=1, K=96, a_ks=1, b_ks=1, epi=4, c_f32=1, splitk=3, opts=opts),
            _row(f"f32-t{tile}-m3-3x{tile}x16-e6", S_M3, tg, dtype=0, M=3, N=tile, K=16, a_ks=1, b_ks=1, epi=6, c_f32=1, opts=opts),
        ]
    # ---- dtype 2, fp32 operands with split-f16 products: the pipelined kernel and the fallback (K % 32 != 0 or split-K) --------------
    for tile, opts in ((64, {}), (128, {"gemm_tile": 128})):
        tg = f"f32 {tile}x{tile} split-f16"
        R += [
            _row(f"split-t{tile}-{tile}x{tile}x32-e0", S_SPLIT, tg, dtype=2, M=tile, N=tile, K=32, opts=opts),
            _row(f"split-t{tile}-{tile + 1}x{tile + 1}x160-e2", S_SPLIT, tg, dtype=2, M=tile + 1, N=tile + 1, K=160, epi=2, pad=(4, 8, 8, 4), opts=opts),
            _row(f"split-t{tile}-1x1x64-e1", S_SPLIT, tg, dtype=2, M=1, N=1, K=64, epi=1, opts=opts),
            _row(f"split-fb-t{tile}-{tile + 1}x{tile}x48-e0", S_SPLIT_FB, tg, dtype=2, M=tile + 1, N=tile, K=48, opts=opts),
            _row(f"split-fb-t{tile}-70x40x50-e3", S_SPLIT_FB, tg, dtype=2, M=70, N=40, K=50, epi=3, opts=opts),
            _row(f"split-fb-t{tile}-{tile}x{tile + 1}x128-e4-s2", S_SPLIT_FB, tg, dtype=2, M=tile, N=tile + 1, K=128, epi=4, c_f32=1, splitk=2, opts=opts),
        ]
    return R


def _grp(id, cfg, ks, probs, site, tag, opts=None, stats_nt=0, drop=0.1, **kw):
    """probs: (M, N, K, epi, c_f32, splitk, pad) per problem"""
    r = dict(id=id, op="group", cfg=cfg, ks=ks, probs=probs, site=site, tag=tag, opts=dict(opts or {}), stats_nt=stats_nt, drop=drop,
             gpu_only=False, checked_by=None)
    r.update(kw)
    return r


PADS = [(0, 0, 8, 16), (64, 8, 0, 8), (8, 64, 16, 8)]


def _group_rows():
    R = []
    KC_P = [(128, 128, 64, 0, 0, 1), (129, 1, 128, 1, 0, 1), (1, 130, 64, 2, 0, 1), (200, 72, 192, 3, 0, 1), (136, 129, 128, 6, 1, 1)]
    KS_P = [(128, 128, 64, 0, 1, 1), (129, 1, 128, 6, 1, 1), (1, 136, 128, 4, 1, 2), (200, 72, 192, 0, 0, 1), (72, 129, 256, 4, 1, 4)]

    def pp(ps, shift=0):
        return [p + (PADS[(i + shift) % len(PADS)],) for i, p in enumerate(ps)]

    # tile_cfg 0 (p5_gemm4_kernel 128x128) at every ring depth, K-contiguous and K-strided; units cross workgroup rounds (g4_wgs 8)
    for nst in (2, 3, 4, 5):
        R.append(_grp(f"g4-128-kc-nst{nst}", 0, 0, pp(KC_P, nst), S_G4, "128xN KC", opts={"g4_nst": nst, "g4_wgs": 8}))
        R.append(_grp(f"g4-128-ks-nst{nst}", 0, 1, pp(KS_P, nst), S_G4, "128x128 KS", opts={"g4_nst": nst, "g4_wgs": 8}))
    R.append(_grp("g4-128-kc-one-wg-round", 0, 0, pp(KC_P[:2]), S_G4, "128xN KC", opts={"g4_wgs": 256}))
    # tile_cfg 1: 256x128 -> p5_gemm5_kernel (gemm_ws bits set, the default), p5_gemm4_kernel with gemm_ws 0
    R.append(_grp("g5-256-kc", 1, 0, pp(KC_P + [(256, 256, 64, 0, 0, 1), (257, 128, 64, 2, 0, 1)]), S_G5, T_WIDE, opts={"g4_wgs": 8}))
    R.append(_grp("g5-256-ks", 1, 1, pp(KS_P + [(256, 128, 64, 6, 1, 1)]), S_G5_KS, T_G5KS, opts={"g4_wgs": 8}))
    R.append(_grp("g4-256-kc", 1, 0, pp(KC_P), S_G4, "256x128 KC", opts={"g4_wgs": 8, "gemm_ws": 0}))
    R.append(_grp("g4-256-ks", 1, 1, pp(KS_P), S_G4, "256x128 KS", opts={"g4_wgs": 8, "gemm_ws": 0}))
    # tile_cfg 2: 128x256 (K-contiguous only); 3: 256x128 loader / compute waves; 4: its 128x128 instance (K-contiguous only)
    R.append(_grp("g4-128x256-kc", 2, 0, pp(KC_P + [(128, 256, 64, 0, 0, 1)]), S_G4, "128xN KC", opts={"g4_wgs": 8}))
    R.append(_grp("g5-cfg3-kc", 3, 0, pp(KC_P, 1), S_G5, T_WIDE, opts={"g4_wgs": 8}))
    R.append(_grp("g5-cfg3-ks", 3, 1, pp(KS_P, 1), S_G5_KS, T_G5KS, opts={"g4_wgs": 8}))
    R.append(_grp("g5-cfg4-kc", 4, 0, pp(KC_P, 2), S_G5_128, T_WS128, opts={"g4_wgs": 8}))
    # folded T5LayerNorm row scale (rowss / rowss_nt) and the output rows' sums of squares (ssq_out) on tile_cfg 3 and 4
    ST_P = [(256, 128, 64, 0, 0, 1), (257, 192, 128, 1, 0, 1), (129, 64, 64, 2, 0, 1), (64, 256, 192, 3, 0, 1)]
    for nt in (4, 8):
        R.append(_grp(f"g5-cfg3-rowss-nt{nt}", 3, 0, pp(ST_P), S_G5, T_WIDE, opts={"g4_wgs": 8}, stats_nt=nt))
        R.append(_grp(f"g5-cfg4-rowss-nt{nt}", 4, 0, pp(ST_P, 1), S_G5_128, T_WS128, opts={"g4_wgs": 8}, stats_nt=nt))
    # epilogues out of scope here, with dedicated tests: gated GELU (5, 7), cross-entropy (8, 9), T5LayerNorm backward (10)
    R.append(_grp("gate", 1, 0, [], S_G5_GATE, "KC + gated-GELU epilogue", checked_by="cases.gemm_gate_case"))
    R.append(_grp("cross-entropy", 1, 0, [], S_G5_CE, "KC + logit-free cross-entropy epilogue", checked_by="cases.ce_free_case"))
    R.append(_grp("norm-bwd", 4, 0, [], S_G5_NBW, "KC 128x128 + T5LayerNorm-backward epilogue", checked_by="cases.gemm_norm_bwd_case"))
    return R


def _skinny_rows():
    R = []
    for dtype in (1, 0):
        for amode in (0, 1):
            K = 512 if (amode == 1 and dtype == 1) else 256      # (amode 1: K = d_model; fp32 rows of 512 do not fit 64-column tiles)
            for nb in (64, 32, 16):
                for epi in ((0, 1, 2, 3, 4) if amode == 0 else (0, 1, 3)):
                    M, N = ((17, 65) if epi in (0, 2) else (1, 64) if epi == 1 else (16, 33))
                    R.append(dict(id=f"skinny-{'bf16' if dtype else 'fp32'}-a{amode}-nb{nb}-{M}x{N}x{K}-e{epi}", op="skinny", dtype=dtype, amode=amode,
                                  M=M, N=N, K=K, epi=epi, pad=(0, 0, 8, 0), alpha=0.75 if epi in (0, 3) else 1.0, opts={"dec_nb": nb},
                                  site=None, tag=None, gpu_only=False, checked_by=None))
    return R


GEMM = _gemm_rows()
GROUP = _group_rows()
SKINNY = _skinny_rows()
ROWS = GEMM + GROUP + SKINNY

# training-scale rows at the T5-small benchmark step (default options, GPU only): encoder 8192 x {512, 1536, 2048} x {512, 2048}, the weight
# gradients 512 x 2048 x 8192 (both operands K-strided), the decoder's 512-row problems
TRAINING = [
    _row("train-enc-8192x1536x512", S_G5, T_WIDE, M=8192, N=1536, K=512, pad=(0, 0, 0, 0)),
    _row("train-enc-8192x2048x512-relu", S_G5, T_WIDE, M=8192, N=2048, K=512, epi=1, pad=(0, 0, 0, 0)),
    _row("train-enc-8192x512x2048-resid", S_G5_128, T_WS128, M=8192, N=512, K=2048, epi=2, pad=(0, 0, 0, 0)),
    _row("train-enc-8192x512x512-resid", S_G5_128, T_WS128, M=8192, N=512, K=512, epi=2, pad=(0, 0, 0, 0)),
    _row("train-enc-8192x2048x2048-mask", S_G5, T_WIDE, M=8192, N=2048, K=2048, epi=3, pad=(0, 0, 0, 0)),
    _row("train-wgrad-512x2048x8192", S_WG4, "bf16 128x128 KS", M=512, N=2048, K=8192, a_ks=1, b_ks=1, epi=4, c_f32=1, splitk=0, pad=(0, 0, 0, 0)),
    _row("train-wgrad-2048x512x8192", S_WG4, "bf16 128x128 KS", M=2048, N=512, K=8192, a_ks=1, b_ks=1, epi=4, c_f32=1, splitk=0, pad=(0, 0, 0, 0)),
    _row("train-dec-512x512x512", S_R32, "", M=512, N=512, K=512, pad=(0, 0, 0, 0)),
    _row("train-dec-512x2048x512-relu", S_SR0, "bf16 64x64 KC", M=512, N=2048, K=512, epi=1, pad=(0, 0, 0, 0)),
    _row("train-dec-512x512x2048-resid", S_R32, "", M=512, N=512, K=2048, epi=2, pad=(0, 0, 0, 0)),
    _row("train-dec-512x1536x512", S_SR0, "bf16 64x64 KC", M=512, N=1536, K=512, pad=(0, 0, 0, 0)),
]


def launch_sites():
    """every launch site the table names"""
    return {r["site"] for r in ROWS + TRAINING if r.get("site")}
