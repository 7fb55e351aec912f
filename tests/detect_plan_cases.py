"""What detection's host-only part (csrc/detect_plan.h) decides, shape by shape: one shape on each side of every rule.

A row is a kind, a name and the arguments of one question, as tests/detect_plan_check.cc reads them from its standard input:

    ws      batch H W channels max_det: the geometry check, the workspace's total and region offsets, its counter words
            (n_holed, arena_used, barrier, max_roots, the count k_clear zeroes), the pixel list's and the arena's size, k_windows' items
    thr     batch H W channels t_low t_high use_high cv_flavour variant, the knobs thr_blocks and seg_h, the matrix-pipe kernel's
            LDS: which threshold kernel runs (or the refusal) with its shape and grid, and ysmr_threshold_workgroups' answer
    chain   batch H W max_det cv_flavour, the knobs collect_blocks, clear_blocks, geo_blocks: the labelling chain's grids
    mean    batch H W and whether the buffers are dword-aligned: the mean-gray branch's kernels, shapes and grids
    levels  inv t_low t_high use_high variant: the matrix-pipe kernel's scales for cv2's taps and its level constants (floats as bits)

EXPECTED holds, per row, the line the program must print.  It was recorded from the commit before detect_plan.h existed, not
derived from the header: that commit's host arithmetic (carve, check_geometry, launch_threshold, ysmr_thr::supported / launch /
choose_scales, ysmr_components_batch's grids, ysmr_mean_threshold_batch's planning) copied expression by expression into a
stand-alone program with the launches replaced by prints, and run on these rows.

tests/test_detect_plan_sanitized.py compares the program's output with EXPECTED on the CPU and asks the loaded library's
ysmr_detect_workspace_bytes for every ws row's total; tests/test_gpu_detect.py runs the small thr rows on the device.
"""
BL, BB, BS = 4, 8, 16      # YSMR_BESIDE_LINK, _BATCH_LINK, _SPLIT_LINK
LDS = 143828               # sizeof(Lds) of thr_mfma.hip


def thr(name, batch, H, W, channels=1, t_low=5, t_high=9, use_high=1, flavour=0, variant=0, thr_blocks=0, seg_h=0, lds=LDS):
    return ("thr", name, (batch, H, W, channels, t_low, t_high, use_high, flavour, variant, thr_blocks, seg_h, lds))


def chain(name, batch, H, W, max_det, flavour=0, collect=0, clear=0, geo=0):
    return ("chain", name, (batch, H, W, max_det, flavour, collect, clear, geo))


def ws(name, batch, H, W, channels, max_det):
    return ("ws", name, (batch, H, W, channels, max_det))


ROWS = [
    # the bench's shapes: 256 and 248 frames of 922 x 1228 beside the batch link, 64 frames with no hint; 4K beside the split link
    ws("ws_bench_256", 256, 922, 1228, 1, 2048), ws("ws_bench_248", 248, 922, 1228, 1, 2048), ws("ws_bench_64", 64, 922, 1228, 1, 2048),
    ws("ws_4k_16", 16, 2160, 3840, 1, 8192), ws("ws_cabi_4", 4, 922, 1228, 1, 2048), ws("ws_smoke", 8, 200, 260, 1, 128),
    ws("ws_1", 1, 1, 1, 1, 1), ws("ws_odd", 3, 7, 13, 3, 64),
    # k_windows' items: H 32 | 33, W 256 | 257
    ws("ws_h32_w256", 2, 32, 256, 1, 16), ws("ws_h33_w256", 2, 33, 256, 1, 16), ws("ws_h32_w257", 2, 32, 257, 1, 16),
    # the arena: sixteen full-width hulls | one full-frame window
    ws("ws_arena_hulls", 2, 100, 400, 1, 16), ws("ws_arena_window", 2, 700, 400, 1, 16),
    # the geometry's limits
    ws("ws_batch_0", 0, 10, 10, 1, 10), ws("ws_h_0", 1, 0, 10, 1, 10), ws("ws_w_0", 1, 10, 0, 1, 10), ws("ws_md_0", 1, 10, 10, 1, 0),
    ws("ws_channels_2", 1, 10, 10, 2, 10), ws("ws_channels_3", 1, 10, 10, 3, 10),
    ws("ws_h_16384", 1, 16384, 8, 1, 8), ws("ws_h_16385", 1, 16385, 8, 1, 8), ws("ws_w_16384", 1, 8, 16384, 1, 8), ws("ws_w_16385", 1, 8, 16385, 1, 8),
    ws("ws_px_at", 24, 10924, 16382, 1, 1), ws("ws_px_over", 24, 10924, 16383, 1, 1), ws("ws_px_2_32", 16, 16384, 16384, 1, 1),
    thr("thr_bench_256", 256, 922, 1228, flavour=BB), thr("thr_bench_248", 248, 922, 1228, flavour=BB), thr("thr_bench_64", 64, 922, 1228),
    thr("thr_4k_16", 16, 2160, 3840, flavour=BS),
    # beside the one-launch link: the strip kernel
    thr("thr_bench_64_beside_link", 64, 922, 1228, flavour=BL), thr("thr_4k_16_strip", 16, 2160, 3840, variant=1),
    # W 60 | 64, H 17 | 18: the matrix-pipe kernel
    thr("thr_h18_w64", 3, 18, 64), thr("thr_h18_w60", 3, 18, 60), thr("thr_h17_w64", 3, 17, 64),
    # levels at +-999 | +-1000
    thr("thr_low_999", 3, 18, 64, t_low=999, t_high=990), thr("thr_low_1000", 3, 18, 64, t_low=1000, t_high=990),
    thr("thr_low_m999", 3, 18, 64, t_low=-999, t_high=-990), thr("thr_low_m1000", 3, 18, 64, t_low=-1000, t_high=-990),
    thr("thr_high_999", 3, 18, 64, t_low=990, t_high=999), thr("thr_high_1000", 3, 18, 64, t_low=990, t_high=1000),
    thr("thr_high_m999", 3, 18, 64, t_low=-990, t_high=-999), thr("thr_high_m1000", 3, 18, 64, t_low=-990, t_high=-1000),
    # use_high with equal levels (gap 0) | one level apart | no second level
    thr("thr_gap_0", 3, 18, 64, t_low=5, t_high=5), thr("thr_gap_1", 3, 18, 64, t_low=5, t_high=6), thr("thr_one_level", 3, 18, 64, t_low=5, t_high=5, use_high=0),
    # W % 4 != 0, W 12 | 16, H 1 | 2: strip | tile
    thr("thr_w_62", 3, 18, 62), thr("thr_w_1229", 2, 100, 1229), thr("thr_h5_w12", 3, 5, 12), thr("thr_h5_w16", 3, 5, 16),
    thr("thr_h1_w16", 3, 1, 16), thr("thr_h2_w16", 3, 2, 16), thr("thr_2x2x16", 2, 2, 16),
    # gap 127 | 128 (where the matrix-pipe kernel does not serve: a small frame; variant 1; three channels)
    thr("thr_gap_127", 3, 5, 16, t_low=5, t_high=132), thr("thr_gap_128", 3, 5, 16, t_low=5, t_high=133),
    thr("thr_gap_127_down", 3, 5, 16, t_low=132, t_high=5), thr("thr_gap_128_down", 3, 5, 16, t_low=133, t_high=5),
    thr("thr_gap_128_one_level", 3, 5, 16, t_low=5, t_high=133, use_high=0),
    thr("thr_gap_127_v1", 3, 18, 64, t_low=5, t_high=132, variant=1), thr("thr_gap_128_v1", 3, 18, 64, t_low=5, t_high=133, variant=1),
    thr("thr_gap_128_mfma", 3, 18, 64, t_low=5, t_high=133),
    # |t| at 99999 | 100000
    thr("thr_low_99999", 3, 18, 64, t_low=99999, t_high=99990), thr("thr_low_100000", 3, 18, 64, t_low=100000, t_high=99990),
    thr("thr_high_m99999", 3, 18, 64, t_low=-99990, t_high=-99999), thr("thr_high_m100000", 3, 18, 64, t_low=-99990, t_high=-100000),
    # three channels
    thr("thr_bgr_bench_64", 64, 922, 1228, channels=3), thr("thr_bgr_h18_w64", 3, 18, 64, channels=3), thr("thr_bgr_w_62", 3, 18, 62, channels=3),
    # variants 1 - 3; 2 and 3 are refused where the matrix-pipe kernel does not serve
    thr("thr_v1", 8, 100, 128, variant=1), thr("thr_v2", 8, 100, 128, variant=2), thr("thr_v3", 8, 100, 128, variant=3),
    thr("thr_v2_refused", 3, 18, 60, variant=2), thr("thr_v3_refused", 3, 17, 64, variant=3), thr("thr_v3_bgr_refused", 3, 18, 64, channels=3, variant=3),
    thr("thr_v2_beside_link", 8, 100, 128, flavour=BL, variant=2), thr("thr_v0_beside_link_and_batch", 8, 100, 128, flavour=BL | BB),
    # batch 7 | 8 | 16: frames dealt to the XCDs
    thr("thr_mfma_b7", 7, 922, 1228), thr("thr_mfma_b8", 8, 922, 1228), thr("thr_mfma_b16", 16, 922, 1228), thr("thr_mfma_b8_h18_w64", 8, 18, 64),
    thr("thr_mfma_b8_248", 8, 922, 1228, flavour=BB), thr("thr_mfma_b7_tall", 7, 1100, 1228), thr("thr_mfma_b8_tall", 8, 1100, 1228),
    thr("thr_strip_b7", 7, 922, 1228, variant=1), thr("thr_strip_b8", 8, 922, 1228, variant=1), thr("thr_strip_b16", 16, 922, 1228, variant=1),
    thr("thr_mfma_b8_h32_w64", 8, 32, 64), thr("thr_mfma_b8_h48_w1236", 8, 48, 1236), thr("thr_strip_b8_h128_w16", 8, 128, 16),
    thr("thr_strip_b8_small", 8, 18, 60), thr("thr_strip_b16_h40_w16", 16, 40, 16), thr("thr_strip_b256", 256, 922, 1228, variant=1),
    # panels: W 1232 | 1236
    thr("thr_w_1232", 2, 64, 1232), thr("thr_w_1236", 2, 64, 1236), thr("thr_w_16384", 1, 64, 16384),
    # strips: 58 | 59 dwords of columns
    thr("thr_strip_w_232", 2, 64, 232, variant=1), thr("thr_strip_w_236", 2, 64, 236, variant=1),
    # the knobs, and a matrix-pipe kernel whose LDS lets two workgroups share a compute unit
    thr("thr_knob_blocks_mfma", 64, 922, 1228, thr_blocks=128), thr("thr_knob_blocks_strip", 64, 922, 1228, variant=1, thr_blocks=512),
    thr("thr_knob_seg_h", 64, 922, 1228, variant=1, seg_h=58), thr("thr_lds_two_per_cu", 64, 922, 1228, lds=70000),
    # the labelling chain
    chain("chain_bench_256", 256, 922, 1228, 2048, BB), chain("chain_bench_248", 248, 922, 1228, 2048, BB), chain("chain_bench_64", 64, 922, 1228, 2048),
    chain("chain_4k_16", 16, 2160, 3840, 8192, BS), chain("chain_smoke", 8, 200, 260, 128),
    # batch 7 | 8: a workgroup per frame for the residue
    chain("chain_b7", 7, 200, 260, 128), chain("chain_b8", 8, 200, 260, 128),
    # max_det 2456 | 2457 with and without YSMR_BESIDE_LINK
    chain("chain_md_2456_beside_link", 64, 922, 1228, 2456, BL), chain("chain_md_2457_beside_link", 64, 922, 1228, 2457, BL),
    chain("chain_md_2456", 64, 922, 1228, 2456), chain("chain_md_2457", 64, 922, 1228, 2457),
    chain("chain_md_2456_beside_split", 64, 922, 1228, 2456, BS),
    # k_rank's grid: 256 ranks per row of blocks, 32 at the most
    chain("chain_md_256", 4, 100, 100, 256), chain("chain_md_257", 4, 100, 100, 257), chain("chain_md_7936", 4, 100, 100, 7936),
    chain("chain_md_7937", 4, 100, 100, 7937), chain("chain_md_8192", 4, 100, 100, 8192), chain("chain_md_8193", 4, 100, 100, 8193),
    # k_windows' grid: fewer than 8 blocks | whole multiples of 8
    chain("chain_windows_7", 1, 224, 1024, 64), chain("chain_windows_8", 1, 256, 1024, 64), chain("chain_windows_9", 1, 288, 1024, 64),
    chain("chain_windows_15", 1, 480, 1024, 64), chain("chain_windows_16", 1, 512, 1024, 64), chain("chain_windows_1", 1, 1, 1, 1),
    chain("chain_knobs", 64, 922, 1228, 2048, BL, 3000, 100, 700),
    # the mean-gray branch
    ("mean", "mean_bench_64", (64, 922, 1228, 1)), ("mean", "mean_bench_256", (256, 922, 1228, 1)), ("mean", "mean_4k_16", (16, 2160, 3840, 1)),
    ("mean", "mean_unaligned", (64, 922, 1228, 0)), ("mean", "mean_w_4", (3, 50, 4, 1)), ("mean", "mean_w_8", (3, 50, 8, 1)),
    ("mean", "mean_w_1229", (3, 50, 1229, 1)), ("mean", "mean_w_248", (3, 50, 248, 1)), ("mean", "mean_w_252", (3, 50, 252, 1)),
    ("mean", "mean_b2000_small", (2000, 10, 10, 1)), ("mean", "mean_1", (1, 1, 1, 1)), ("mean", "mean_b1_tall", (1, 16384, 8, 1)),
    ("mean", "mean_b1024", (1024, 64, 64, 1)), ("mean", "mean_b1025", (1025, 64, 64, 1)), ("mean", "mean_h_4", (4000, 4, 16, 1)),
    # the matrix-pipe kernel's scales (cv2's sigma-2 taps) and level constants
    ("levels", "levels_bench", (1, 5, 9, 1, 0)), ("levels", "levels_binary", (0, 5, 9, 1, 0)), ("levels", "levels_down", (1, 9, 5, 1, 0)),
    ("levels", "levels_binary_down", (0, 9, 5, 1, 0)), ("levels", "levels_one", (1, 5, 9, 0, 0)), ("levels", "levels_half_scale", (1, 5, 9, 1, 1)),
    ("levels", "levels_exact", (1, 5, 9, 1, 2)), ("levels", "levels_negative", (0, -999, 999, 1, 0)),
]

EXPECTED = {
    'ws_bench_256':
        'total=511699456 offsets=0,256,33280,34304,144957952,144990720,147087872,149185024,157573632,159670784,161767936,170156544,172253696,182739456,473688576 counters=8192,8193,8194,8195,8200 pixel_cap=36230912 arena_floats=72737280 win_items=37120',
    'ws_bench_248':
        'total=495710208 offsets=0,256,32256,33280,140428288,140461056,142492672,144524288,152650752,154682368,156713984,164840448,166872064,177030144,458887168 counters=7936,7937,7938,7939,7944 pixel_cap=35098696 arena_floats=70464240 win_items=35960',
    'ws_bench_64':
        'total=127949824 offsets=0,256,8704,8960,36239872,36272640,36796928,37321216,39418368,39942656,40466944,42564096,43088384,45709824,118447104 counters=2048,2049,2050,2051,2056 pixel_cap=9057728 arena_floats=18184320 win_items=9280',
    'ws_4k_16':
        'total=225442304 offsets=0,256,2560,2816,66358016,66390784,66915072,67439360,69536512,70060800,70585088,72682240,73206528,75827968,208730624 counters=512,513,514,515,520 pixel_cap=16588800 arena_floats=33225616 win_items=16320',
    'ws_cabi_4':
        'total=8028672 offsets=0,256,1024,1280,2265856,2298624,2331392,2364160,2495232,2528000,2560768,2691840,2724608,2888448,7434752 counters=128,129,130,131,136 pixel_cap=566108 arena_floats=1136520 win_items=580',
    'ws_smoke':
        'total=1769984 offsets=0,256,1536,1792,209920,242688,246784,250880,267264,271360,275456,291840,295936,316416,1655296 counters=256,257,258,259,264 pixel_cap=52000 arena_floats=334720 win_items=112',
    'ws_1':
        'total=38656 offsets=0,256,512,768,1024,33792,34048,34304,34560,34816,35072,35328,35584,35840,37632 counters=32,33,34,35,40 pixel_cap=1 arena_floats=400 win_items=1',
    'ws_odd':
        'total=78848 offsets=0,256,768,1024,1280,34048,34816,35584,38656,39424,40192,43264,44032,47872,75776 counters=96,97,98,99,104 pixel_cap=35 arena_floats=6960 win_items=3',
    'ws_h32_w256':
        'total=376832 offsets=0,256,768,1024,9216,41984,42240,42496,43008,43264,43520,44032,44288,45056,374784 counters=64,65,66,67,72 pixel_cap=2048 arena_floats=82400 win_items=2',
    'ws_h33_w256':
        'total=379136 offsets=0,256,768,1024,9472,42240,42496,42752,43264,43520,43776,44288,44544,45312,375040 counters=64,65,66,67,72 pixel_cap=2112 arena_floats=82400 win_items=4',
    'ws_h32_w257':
        'total=380416 offsets=0,256,768,1024,9472,42240,42496,42752,43264,43520,43776,44288,44544,45312,376320 counters=64,65,66,67,72 pixel_cap=2056 arena_floats=82720 win_items=4',
    'ws_arena_hulls':
        'total=607488 offsets=0,256,768,1024,41216,73984,74240,74496,75008,75264,75520,76032,76288,77056,591104 counters=64,65,66,67,72 pixel_cap=10000 arena_floats=128480 win_items=16',
    'ws_arena_window':
        'total=971520 offsets=0,256,768,1024,281088,313856,314112,314368,314880,315136,315392,315904,316160,316928,881408 counters=64,65,66,67,72 pixel_cap=70000 arena_floats=141102 win_items=88',
    'ws_batch_0': 'error=positive',
    'ws_h_0': 'error=positive',
    'ws_w_0': 'error=positive',
    'ws_md_0': 'error=positive',
    'ws_channels_2': 'error=channels',
    'ws_channels_3':
        'total=44288 offsets=0,256,512,768,1024,33792,34048,34304,34560,34816,35072,35328,35584,35840,43264 counters=32,33,34,35,40 pixel_cap=13 arena_floats=1840 win_items=1',
    'ws_h_16384':
        'total=789504 offsets=0,256,512,768,66304,99072,99328,99584,99840,100096,100352,100608,100864,101120,265216 counters=32,33,34,35,40 pixel_cap=16384 arena_floats=40965 win_items=512',
    'ws_h_16385': 'error=too_large',
    'ws_w_16384':
        'total=10653440 offsets=0,256,512,768,66304,99072,99328,99584,99840,100096,100352,100608,100864,101120,10587904 counters=32,33,34,35,40 pixel_cap=16384 arena_floats=2621680 win_items=64',
    'ws_w_16385': 'error=too_large',
    'ws_px_at':
        'total=6981720576 offsets=0,256,3584,3840,2147487488,2147520256,2147520512,2147520768,2147521280,2147521536,2147521792,2147522304,2147522560,2147523072,6443801088 counters=768,769,770,771,776 pixel_cap=536870904 arena_floats=1074069504 win_items=525312',
    'ws_px_over': 'error=too_large',
    'ws_px_2_32': 'error=too_large',
    'thr_bench_256': 'workgroups=248 kernel=mfma variant=0 panels=1 panel_w=1232 grid=248 by_xcd=1 start_rows=48',
    'thr_bench_248': 'workgroups=248 kernel=mfma variant=0 panels=1 panel_w=1232 grid=248 by_xcd=1 start_rows=0',
    'thr_bench_64': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=256 by_xcd=1 start_rows=0',
    'thr_4k_16': 'workgroups=160 kernel=mfma variant=0 panels=4 panel_w=960 grid=160 by_xcd=1 start_rows=48',
    'thr_bench_64_beside_link': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=116 segs_y=8 blocks=768 by_xcd=1',
    'thr_4k_16_strip': 'workgroups=256 kernel=strip strips_x=17 out_lanes=57 seg_h=197 segs_y=11 blocks=748 by_xcd=0',
    'thr_h18_w64': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_h18_w60': 'workgroups=256 kernel=strip strips_x=1 out_lanes=15 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_h17_w64': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_low_999': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_low_1000': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_low_m999': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_low_m1000': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_high_999': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_high_1000': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_high_m999': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_high_m1000': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_gap_0': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_gap_1': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_one_level': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_w_62': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_w_1229': 'workgroups=256 kernel=tile grid=20x4x2',
    'thr_h5_w12': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_h5_w16': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_h1_w16': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_h2_w16': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_2x2x16': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_gap_127': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_gap_128': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_gap_127_down': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_gap_128_down': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_gap_128_one_level': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_gap_127_v1': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_gap_128_v1': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_gap_128_mfma': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=1 by_xcd=0 start_rows=48',
    'thr_low_99999': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_low_100000': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_high_m99999': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_high_m100000': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_bgr_bench_64': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=116 segs_y=8 blocks=768 by_xcd=1',
    'thr_bgr_h18_w64': 'workgroups=256 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=1 blocks=1 by_xcd=0',
    'thr_bgr_w_62': 'workgroups=256 kernel=tile grid=1x1x3',
    'thr_v1': 'workgroups=256 kernel=strip strips_x=1 out_lanes=32 seg_h=32 segs_y=4 blocks=8 by_xcd=1',
    'thr_v2': 'workgroups=256 kernel=mfma variant=1 panels=1 panel_w=128 grid=25 by_xcd=0 start_rows=48',
    'thr_v3': 'workgroups=256 kernel=mfma variant=2 panels=1 panel_w=128 grid=25 by_xcd=0 start_rows=48',
    'thr_v2_refused': 'workgroups=256 kernel=refused',
    'thr_v3_refused': 'workgroups=256 kernel=refused',
    'thr_v3_bgr_refused': 'workgroups=256 kernel=refused',
    'thr_v2_beside_link': 'workgroups=256 kernel=mfma variant=1 panels=1 panel_w=128 grid=25 by_xcd=0 start_rows=48',
    'thr_v0_beside_link_and_batch': 'workgroups=248 kernel=strip strips_x=1 out_lanes=32 seg_h=32 segs_y=4 blocks=8 by_xcd=1',
    'thr_mfma_b7': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=201 by_xcd=0 start_rows=48',
    'thr_mfma_b8': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=230 by_xcd=0 start_rows=48',
    'thr_mfma_b16': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=256 by_xcd=1 start_rows=0',
    'thr_mfma_b8_h18_w64': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=4 by_xcd=0 start_rows=48',
    'thr_mfma_b8_248': 'workgroups=248 kernel=mfma variant=0 panels=1 panel_w=1232 grid=230 by_xcd=0 start_rows=48',
    'thr_mfma_b7_tall': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=240 by_xcd=0 start_rows=48',
    'thr_mfma_b8_tall': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=256 by_xcd=1 start_rows=0',
    'thr_strip_b7': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=32 segs_y=29 blocks=305 by_xcd=0',
    'thr_strip_b8': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=32 segs_y=29 blocks=348 by_xcd=0',
    'thr_strip_b16': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=32 segs_y=29 blocks=696 by_xcd=1',
    'thr_mfma_b8_h32_w64': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=64 grid=8 by_xcd=1 start_rows=0',
    'thr_mfma_b8_h48_w1236': 'workgroups=256 kernel=mfma variant=0 panels=2 panel_w=624 grid=24 by_xcd=1 start_rows=48',
    'thr_strip_b8_h128_w16': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=4 blocks=8 by_xcd=1',
    'thr_strip_b8_small': 'workgroups=256 kernel=strip strips_x=1 out_lanes=15 seg_h=32 segs_y=1 blocks=2 by_xcd=0',
    'thr_strip_b16_h40_w16': 'workgroups=256 kernel=strip strips_x=1 out_lanes=4 seg_h=32 segs_y=2 blocks=8 by_xcd=1',
    'thr_strip_b256': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=461 segs_y=2 blocks=768 by_xcd=1',
    'thr_w_1232': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=4 by_xcd=0 start_rows=0',
    'thr_w_1236': 'workgroups=256 kernel=mfma variant=0 panels=2 panel_w=624 grid=8 by_xcd=0 start_rows=0',
    'thr_w_16384': 'workgroups=256 kernel=mfma variant=0 panels=14 panel_w=1184 grid=28 by_xcd=0 start_rows=0',
    'thr_strip_w_232': 'workgroups=256 kernel=strip strips_x=1 out_lanes=58 seg_h=32 segs_y=2 blocks=1 by_xcd=0',
    'thr_strip_w_236': 'workgroups=256 kernel=strip strips_x=2 out_lanes=30 seg_h=32 segs_y=2 blocks=2 by_xcd=0',
    'thr_knob_blocks_mfma': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=128 by_xcd=1 start_rows=0',
    'thr_knob_blocks_strip': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=185 segs_y=5 blocks=480 by_xcd=1',
    'thr_knob_seg_h': 'workgroups=256 kernel=strip strips_x=6 out_lanes=52 seg_h=58 segs_y=16 blocks=768 by_xcd=1',
    'thr_lds_two_per_cu': 'workgroups=256 kernel=mfma variant=0 panels=1 panel_w=1232 grid=512 by_xcd=1 start_rows=0',
    'chain_bench_256': 'clear=512 windows=8192 residue=frames:256 rank=256x8 geometry=1664',
    'chain_bench_248': 'clear=512 windows=8192 residue=frames:248 rank=248x8 geometry=1664',
    'chain_bench_64': 'clear=512 windows=2320 residue=frames:64 rank=64x8 geometry=1664',
    'chain_4k_16': 'clear=512 windows=2048 residue=frames:16 rank=16x32 geometry=1664',
    'chain_smoke': 'clear=512 windows=24 residue=frames:8 rank=8x1 geometry=1664',
    'chain_b7': 'clear=512 windows=24 residue=grid:128 rank=7x1 geometry=1664',
    'chain_b8': 'clear=512 windows=24 residue=frames:8 rank=8x1 geometry=1664',
    'chain_md_2456_beside_link': 'clear=512 windows=1024 residue=frames:64 rank=64x10 geometry=640',
    'chain_md_2457_beside_link': 'clear=512 windows=2048 residue=frames:64 rank=64x10 geometry=1664',
    'chain_md_2456': 'clear=512 windows=2320 residue=frames:64 rank=64x10 geometry=1664',
    'chain_md_2457': 'clear=512 windows=2320 residue=frames:64 rank=64x10 geometry=1664',
    'chain_md_2456_beside_split': 'clear=512 windows=2048 residue=frames:64 rank=64x10 geometry=1664',
    'chain_md_256': 'clear=512 windows=4 residue=grid:128 rank=4x1 geometry=1664',
    'chain_md_257': 'clear=512 windows=4 residue=grid:128 rank=4x2 geometry=1664',
    'chain_md_7936': 'clear=512 windows=4 residue=grid:128 rank=4x31 geometry=1664',
    'chain_md_7937': 'clear=512 windows=4 residue=grid:128 rank=4x32 geometry=1664',
    'chain_md_8192': 'clear=512 windows=4 residue=grid:128 rank=4x32 geometry=1664',
    'chain_md_8193': 'clear=512 windows=4 residue=grid:128 rank=4x32 geometry=1664',
    'chain_windows_7': 'clear=512 windows=7 residue=grid:128 rank=1x1 geometry=1664',
    'chain_windows_8': 'clear=512 windows=8 residue=grid:128 rank=1x1 geometry=1664',
    'chain_windows_9': 'clear=512 windows=8 residue=grid:128 rank=1x1 geometry=1664',
    'chain_windows_15': 'clear=512 windows=8 residue=grid:128 rank=1x1 geometry=1664',
    'chain_windows_16': 'clear=512 windows=16 residue=grid:128 rank=1x1 geometry=1664',
    'chain_windows_1': 'clear=512 windows=1 residue=grid:128 rank=1x1 geometry=1664',
    'chain_knobs': 'clear=100 windows=2320 residue=frames:64 rank=64x8 geometry=828',
    'mean_bench_64': 'parts=16 sum_blocks=1024 kernel=strip strips_x=5 out_lanes=62 seg_h=49 segs_y=19 blocks=768',
    'mean_bench_256': 'parts=4 sum_blocks=1024 kernel=strip strips_x=5 out_lanes=62 seg_h=58 segs_y=16 blocks=768',
    'mean_4k_16': 'parts=64 sum_blocks=1024 kernel=strip strips_x=16 out_lanes=60 seg_h=60 segs_y=36 blocks=768',
    'mean_unaligned': 'parts=16 sum_blocks=1024 kernel=thread groups_x=307 segs_y=29 blocks=1024',
    'mean_w_4': 'parts=1 sum_blocks=3 kernel=thread groups_x=1 segs_y=2 blocks=1',
    'mean_w_8': 'parts=1 sum_blocks=3 kernel=strip strips_x=1 out_lanes=2 seg_h=8 segs_y=7 blocks=6',
    'mean_w_1229': 'parts=16 sum_blocks=48 kernel=thread groups_x=308 segs_y=2 blocks=8',
    'mean_w_248': 'parts=4 sum_blocks=12 kernel=strip strips_x=1 out_lanes=62 seg_h=8 segs_y=7 blocks=6',
    'mean_w_252': 'parts=4 sum_blocks=12 kernel=strip strips_x=2 out_lanes=32 seg_h=8 segs_y=7 blocks=11',
    'mean_b2000_small': 'parts=1 sum_blocks=1024 kernel=thread groups_x=3 segs_y=1 blocks=24',
    'mean_1': 'parts=1 sum_blocks=1 kernel=thread groups_x=1 segs_y=1 blocks=1',
    'mean_b1_tall': 'parts=32 sum_blocks=32 kernel=strip strips_x=1 out_lanes=2 seg_h=8 segs_y=2048 blocks=512',
    'mean_b1024': 'parts=1 sum_blocks=1024 kernel=strip strips_x=1 out_lanes=16 seg_h=22 segs_y=3 blocks=768',
    'mean_b1025': 'parts=1 sum_blocks=1024 kernel=strip strips_x=1 out_lanes=16 seg_h=32 segs_y=2 blocks=513',
    'mean_h_4': 'parts=1 sum_blocks=1024 kernel=strip strips_x=1 out_lanes=4 seg_h=8 segs_y=1 blocks=768',
    'levels_bench':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=c21e5efd neg_x_mul=421d8000 k_first=c3bb0800 d2=431d8000 sh=6,2020202,7,1010101',
    'levels_binary':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=421e5efd neg_x_mul=c21d8000 k_first=43589000 d2=431d8000 sh=7,1010101,6,2020202',
    'levels_down':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=c21e5efd neg_x_mul=421d8000 k_first=c3bb0800 d2=431d8000 sh=7,1010101,6,2020202',
    'levels_binary_down':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=421e5efd neg_x_mul=c21d8000 k_first=43589000 d2=431d8000 sh=6,2020202,7,1010101',
    'levels_one':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=c21e5efd neg_x_mul=421d8000 k_first=c3589000 d2=80000000 sh=7,1010101,6,2020202',
    'levels_half_scale':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=c19e5efd neg_x_mul=419d8000 k_first=c33b0800 d2=429d8000 sh=6,2020202,7,1010101',
    'levels_exact':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=c21e5efd neg_x_mul=421d8000 k_first=c3bb0800 d2=431d8000 sh=6,2020202,7,1010101',
    'levels_negative':
        's=0.99450000000000005 S=39.375 bound=0.042265559633839371 col_scale=3f7e978d row_scale=421e5efd neg_x_mul=c21d8000 k_first=c71993f0 d2=4799a7a0 sh=7,1010101,6,2020202',
}


def line_of(kind, name, args):
    """A row as detect_plan_check reads it from its standard input."""
    return f"{kind} {name} {' '.join(str(a) for a in args)}"
