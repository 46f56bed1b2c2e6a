"""The tile rule of the fused ResBlock2 kernel, restated from dict_tts_amd/csrc/rb2x.h / rb2x.hip (rb2x_halo, rb2x_guard, rb2x_lds_bytes,
rb2x_supported, rb2x_launch_el) for the tests that build shapes from it."""
LDS = 160 * 1024
BASE_ROWS = {32: 512, 64: 512, 128: 256, 256: 128}
WIDE_ROWS = {32: 1024, 64: 512, 128: 384, 256: 192}
TIME_WAVES = {(32, 512): 4, (32, 1024): 8, (64, 512): 4, (128, 256): 2, (128, 384): 2, (256, 128): 1, (256, 192): 1}


def halo(k, d0, d1):
    return (k - 1) // 2 * (d0 + d1)


def guard(k, d0, d1):
    return (k + 1) // 2 * max(d0, d1)


def lds_bytes(C, W, k, d0, d1, wav):
    act = (W + 2 * guard(k, d0, d1)) * (C * 2 + 16)
    if not wav:
        return act
    return max((W - 2 * halo(k, d0, d1)) * C * 4, act) + TIME_WAVES[(C, W)] * 32 * (C * 4 + 16)


def table_bytes(B):
    return (3 * B + 2) * 4


def supported(C, k, d0, d1, max_batch=2048):
    if C not in BASE_ROWS or k % 2 == 0 or k < 3 or k > 11 or d0 < 1 or d1 < 1:
        return False
    W = BASE_ROWS[C]
    if W - 2 * halo(k, d0, d1) < (38 if C == 32 else 32):
        return False
    return lds_bytes(C, W, k, d0, d1, C == 32) + table_bytes(max_batch) <= LDS


def tile_rows(C, k, d0, d1, B, wav):
    """output rows per tile of the launch rb2x_launch_el picks for a batch of B utterances (with the fused conv_post: 6 less)"""
    h = halo(k, d0, d1)
    wide = (k >= 7) if C == 32 else (C >= 128 and h >= 16)
    chain = ([WIDE_ROWS[C]] if wide else []) + [BASE_ROWS[C]]
    for W in chain:
        tto = W - 2 * h - (6 if wav else 0)
        if tto >= 32 and lds_bytes(C, W, k, d0, d1, wav) + table_bytes(B) <= LDS:
            return tto
    raise ValueError((C, k, d0, d1, B, wav))


def stage_tiles(cfg, B):
    """{launch: output rows per tile} of the LAST stage's ResBlock2 launches"""
    C = cfg["upsample_initial_channel"] >> len(cfg["upsample_rates"])
    nk = len(cfg["resblock_kernel_sizes"])
    out = {}
    for j, (k, (d0, d1)) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
        wav = C == 32 and j == nk - 1 and nk >= 2
        out[f"rb2x<{C}> k={k} d=({d0},{d1}){' +post' if wav else ''}"] = tile_rows(C, k, d0, d1, B, wav)
    return out


def largest_pair(C, k):
    """the admitted dilation pair with the largest halo (ties: the larger second dilation)"""
    best = None
    for d0 in range(1, 200):
        for d1 in range(1, 200):
            if supported(C, k, d0, d1):
                key = (halo(k, d0, d1), d1)
                if best is None or key > best[0]:
                    best = (key, (d0, d1))
    return best[1]
