"""Geometries between the two the suite grew up on (8 x 8 and 64 x 64 latents): the cases of the 192 / 320 / 384 px model tests, and
`expected_paths`, a restatement of the predicates that decide which kernel a block of the denoising UNet launches.

The predicates are written out again here on purpose (token counts, sides, channel widths: nothing is imported from mmgt_amd), so that
a gate that changes in mmgt_amd/unet3d.py or mmgt_amd/hip.py without the same change here fails the launch-count tests."""
import torch

from tests import golden_cases as gc

_BASE = gc.UNET_CASES["full_cfg1"]

# name -> case of tests/golden_cases.unet_inputs (full width, CFG pair)
UNET_GEOMETRY = {
    "lat48_f12": dict(_BASE, frames=12, latent=48, timestep=499),     # 384 px: every level-0 gate on, the 12 x 12 level's fused legs off
    "lat24_f24": dict(_BASE, frames=24, latent=24, timestep=499),     # 192 px: the fused temporal leg alone between unfused neighbours
    "lat40_f5": dict(_BASE, frames=5, latent=40, timestep=499),       # 320 px: every geometry gate off; 20 / 10 / 5 wide levels
}

# the reference's own UNet at a 40 x 40 latent (tests/golden/unet3d_full_lat40.npz, tools/refgen/gen_golden.py --only geometry)
GOLDEN_LAT40 = dict(_BASE, frames=2, latent=40, timestep=499)

REFNET_LATENTS = (40, 48)
PIPELINE_320 = dict(latent=40, frames=5, steps=2)                      # 320 x 320 px, one window of 5 frames
VAE_RECT = (40, 24)                                                    # latent rows x columns -> 320 x 192 px

PATHS = ("mmgt_temporal_leg320", "mmgt_gn_silu_conv3x3_unet", "mmgt_gn_stats_finalize_unet", "mmgt_rowgemm320", "mmgt_ff_fused",
         "mmgt_ff_fused_po", "mmgt_conv1x1_cat_nhwc", "mmgt_conv_taps_gather")

WIDTHS = (320, 640, 1280, 1280)


def expected_paths(latent, frames, dtype):
    """Launches per forward of `UNet3DConditionModel` on a CFG pair (2, 4, frames, latent, latent) at the default switches, by entry point.

    Structure (SD-1.5 widths, two layers per block): level l has side latent / 2^l and width WIDTHS[l].  Level 0 holds 5 resnets, 5
    spatial transformers, 5 motion modules (down 2 + up 3) and 2 audio modules; levels 1 and 2 the same; level 3 holds 7 resnets (down 2,
    mid 2, up 3) and 6 motion modules, and the mid block's spatial transformer.  The first audio module of a level takes the width of the
    level above as its inner width, so the one at level 1 is 320 wide inside (its proj_in / proj_out are 640 <-> 320).
    Every fused path is bf16 only: in fp32 mode all counts are zero.  Holds for one window whose operands stay below the 2 GiB a kernel
    addresses (up to 24 frames of 64 x 64 latents), where no launch is split into runs of rows."""
    n = {k: 0 for k in PATHS}
    if dtype != torch.bfloat16:
        return n
    side = [latent >> l for l in range(4)]
    tok = [s * s for s in side]
    nb = 2 * frames                                     # images per forward
    n0, n1 = tok[0], tok[1]
    rows128 = n0 % 128 == 0                             # the row-stationary launches cut a level-0 image into runs of 128 tokens

    # the fused temporal leg: both attention legs of the five 320-wide motion modules (windows of 12 or 24 frames, whole 4-wave tasks)
    tleg = frames in (12, 24) and n0 % (4 * 48 // frames) == 0 and 2 * frames * n0 * 640 < (1 << 31)
    n["mmgt_temporal_leg320"] = 10 if tleg else 0

    # GroupNorm -> SiLU -> conv3x3 as one launch: the 320-wide (level 0: 5) and 1280-wide resnets (level 2: down 2 + up 3, level 3: 7) whose
    # side tiles into 16 x 16 pixels, two legs each; the 640-wide level is not in the default `rconv` mask
    fused = {0: 5 if side[0] % 16 == 0 else 0, 2: 5 if side[2] % 16 == 0 else 0, 3: 7 if side[3] % 16 == 0 else 0}
    n["mmgt_gn_silu_conv3x3_unet"] = 2 * sum(fused.values())
    # a table from an epilogue: norm2 of every fused resnet (conv1), and the `norm` of the level-0 spatial transformer behind a fused
    # 320-wide resnet where that block's GroupNorm -> proj_in is one launch (more than 256 tokens, whole runs of 128)
    proj_in_fused = n0 > 256 and rows128
    n["mmgt_gn_stats_finalize_unet"] = sum(fused.values()) + (fused[0] if proj_in_fused else 0)

    r = 3                                               # LayerNorm -> q of the three audio branches: the 320-wide audio modules (level 0: 2, level 1: 1)
    if proj_in_fused:
        r += 5 + 2 + 5                                  # GroupNorm -> proj_in: level-0 spatial, audio and motion blocks
    if rows128:
        r += 5 + 2                                      # LayerNorm -> q | k | V^T: level-0 spatial and audio self-attention
        r += 0 if tleg else 10                          # LayerNorm + pe -> q | k | v of the level-0 temporal legs, unless the whole leg is fused
        r += 1                                          # conv_norm_out -> SiLU -> the nine taps of conv_out
    if n1 % 128 == 0:
        r += 1                                          # the 320-wide audio module at level 1
    n["mmgt_rowgemm320"] = r
    n["mmgt_conv_taps_gather"] = 1 if rows128 else 0

    # LayerNorm -> FeedForward -> proj_out in one launch: the twelve 320-wide blocks of level 0; the 320-wide audio module of level 1 ends in
    # a 320 -> 640 proj_out, so its FeedForward is fused without it.  Neither depends on the geometry.
    n["mmgt_ff_fused_po"] = 12
    n["mmgt_ff_fused"] = 1

    # two-source 1 x 1 conv: (a) ff2 + proj_out of every wider block whose proj_out is square: spatial 5 + 5 + 1 (mid), audio 1 + 1 (the
    # second of levels 1 and 2), motion 5 + 5 + 6; (b) conv_shortcut over [x | skip] of the up-block resnets from 6144 rows up
    cat = 11 + 2 + 16
    cat += 3 * sum(1 for level in range(4) if nb * tok[level] >= 6144)      # three up-block resnets per level
    n["mmgt_conv1x1_cat_nhwc"] = cat
    return n


def refnet_fused_levels(latent):
    """Levels at which the ReferenceNet's resnets run the fused GroupNorm -> SiLU -> conv3x3 legs (the same gate as the UNet's): the
    resnets there are down 2 + up 3 at levels 0 and 2, and 7 at level 3."""
    return tuple(l for l in (0, 2, 3) if (latent >> l) % 16 == 0)


def vae_gnconv_launches(h, w):
    """`mmgt_gn_silu_conv3x3` launches of one bf16 decode of an h x w latent.  The fused launch serves 128 or 256 input channels (one launch
    per 128 output channels) on levels whose sides are multiples of 16 with more than 256 pixels: the 256-wide level at 4x (resnet 0: conv2,
    resnets 1 and 2: both convs; two launches each), the 128-wide level at 8x (six convs) and conv_out.  The 512-wide levels (1x, 2x and
    conv1 of the first 256-wide resnet) have no fused form, whatever their sides."""
    on = lambda s: (h * s) % 16 == 0 and (w * s) % 16 == 0 and h * s * w * s > 256
    return (5 * 2 if on(4) else 0) + (6 + 1 if on(8) else 0)
