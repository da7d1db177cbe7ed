"""The split-K rule as `ops.py` stated it before the library took it over (csrc/igemm.hip: splitk_pick): a frozen copy of its two
functions and of the selection branch of `ops.conv(splitk=None)`, kept as the reference the library's DC_SPLITK_AUTO is held to
(tests/test_conv_route.py, tests/test_gpu_ops.py).  Not product code: nothing under the package imports it, and a re-fit of the
rule changes the library and then, knowingly, this file."""
import math


def _pick_splitk(m, cout, kt, units=None, rows_per_image=0):
    """Split the K loop over workgroups when the output has too few tiles to fill 256 CUs and K is long (the
    weight-streaming layers at 8x8 / 16x16).  Each split stores its partial tile into its own fp32 slab and a finish
    pass sums the slabs (m*cout*4 bytes written and read once per split: cheap next to the weight stream, and
    deterministic).  `units` = what the launched kernel partitions (64-channel chunks for the halo-tile 3x3 kernel,
    64-wide K steps otherwise); an even partition is preferred, so the split is a divisor of `units`."""
    tile3 = units is not None
    units = kt if units is None else units
    bn = 160 if cout % 160 == 0 else 128
    tiles = math.ceil(m / 64) * math.ceil(cout / bn)
    # (per-shape sweep of every decode shape at model batches 32 and 2, round 3: short K loops are split only at tiny m, where nothing
    # else fills the chip; a 1x1 launch with >= 2048 rows needs >= 128 K steps before a split pays)
    if tiles >= 512 or (kt < 64 and (m >= 2048 or kt < 32)) or (not tile3 and m >= 2048 and kt < 128):
        return 1
    divs = [s for s in range(1, min(units, 20) + 1) if units % s == 0 and kt // s >= 8]
    target = 1024 if m >= 2048 else 256      # measured (tools/bench_splitk.py): ~1 workgroup per CU at small m, 2+ above
    if tile3 and rows_per_image >= 1024:     # 32x32 and 64x64 maps of a one- or two-frame decode (the halo-tile kernel's own pixel tiles
        target = 256                         # already give 64-256 workgroups): one workgroup per CU, not four (38 -> 26 us at 2x32x32x640)
    for s in divs:
        if tiles * s >= target:
            return s
    return divs[-1] if divs else 1


def _pick_splitk_strided(m, cout, kt):
    """The stride-2 Downsample2D convs (gather GEMM, 64-row tiles): measured per shape (tools/ab/bench_down.py, model batches 32 and 2) the
    best split is the smallest divisor of the K steps that yields ~1024 workgroups with at least 8 steps each — 1 / 2 / 4 at the three
    levels of a 16-frame step (the general rule gave 1 / 1 / 3: 136 -> 109 us at 32x32x640), 5 at the top level of a one-frame decode
    (53 -> 25 us), which the general rule leaves unsplit because its K loop is short."""
    bn = 160 if cout % 160 == 0 else 128
    tiles = math.ceil(m / 64) * math.ceil(cout / bn)
    divs = [s for s in range(1, min(kt, 20) + 1) if kt % s == 0 and kt // s >= 8]
    for s in divs:
        if tiles * s >= 1024:
            return s
    return divs[-1] if divs else 1


def pick(m, cin, cout, k, stride, rows_per_image, tile_kernel, geglu=False, unsplit_epilogue=False):
    """The selection branch of `ops.conv(splitk=None)`: m = N*Ho*Wo output rows, rows_per_image = Ho*Wo, unsplit_epilogue = `ln_stats`
    or `stats_out` is set, tile_kernel() = "the library routes this launch, at split 1 and without gn_part_out, to conv3x3_tile"
    (asked only for a 3x3 stride-1 launch, as the branch asked `conv_route`)."""
    kt = (9 if k == 3 else 1) * (cin // 64)
    if unsplit_epilogue:
        return 1
    if k == 3 and stride == 2 and not geglu:
        return _pick_splitk_strided(m, cout, kt)
    elif geglu:
        return 1
    else:                               # the halo-tile 3x3 kernel splits 64-channel chunks, the others 64-wide K steps
        tile3 = k == 3 and stride == 1 and tile_kernel()
        return _pick_splitk(m, cout, kt, cin // 64 if tile3 else None, rows_per_image=rows_per_image)
