"""The tile rule of the narrow whole-ResBlock1 kernel (C = 16 / 8), restated from dict_tts_amd/csrc/rbn.h / rbn.hip (rbn_padded_taps, rbn_guard,
rbn_lds_bytes, rbn_supported, rbn_launch_el) for the tests that build shapes from it."""
LDS = 160 * 1024
ROWS = (1024, 512, 256)


def _cdiv(a, b):
    return -(-a // b)


def padded_taps(C, k):
    tps = 32 // C
    return _cdiv(k, tps) * tps


def halo(k, dils):
    return max((k - 1) // 2 * (sum(dils) + 3), 6 * (k - 1))   # rblock.h rblock_halo_of


def guard(C, k, dils):
    return (padded_taps(C, k) - 1 - (k - 1) // 2) * max(1, *dils)


def lds_bytes(C, W, k, dils, wav):
    steps = padded_taps(C, k) // (32 // C)
    return 6 * steps * 1024 + (W + 2 * guard(C, k, dils)) * C * 2 + ((W - 2 * halo(k, dils)) * C * 4 if wav else 0)


def table_bytes(B):
    return (3 * B + 2) * 4


def supported(C, k, dils, max_batch=2048):
    if C not in (16, 8) or k % 2 == 0 or k < 3 or k > 11 or min(dils) < 1:
        return False
    if ROWS[2] - 2 * halo(k, dils) - 6 < 32:
        return False
    return lds_bytes(C, ROWS[2], k, dils, True) + table_bytes(max_batch) <= LDS


def tile_rows(C, k, dils, B, L, wav, cus):
    """output rows per tile of the launch rbn_launch_el picks for B utterances padded to L stage rows on a device of `cus` compute units
    (with the fused conv_post: 6 less): 1024-row tiles, 512 while those leave more than half the CUs without a tile, 256 while 512 still do;
    a tile that does not fit (LDS with the tile table, fewer than 32 rows left) falls through to the next smaller one"""
    h = halo(k, dils)

    def tto(W):
        return W - 2 * h - (6 if wav else 0)

    def few(W):
        return tto(W) >= 32 and 2 * B * _cdiv(L, tto(W)) <= cus

    first = (2 if few(ROWS[1]) else 1) if few(ROWS[0]) else 0
    for W in ROWS[first:]:
        if tto(W) >= 32 and lds_bytes(C, W, k, dils, wav) + table_bytes(B) <= LDS:
            return tto(W)
    raise ValueError((C, k, dils, B, L, wav))


def stage_tiles(cfg, B, L, cus):
    """{launch: output rows per tile} of the LAST stage's ResBlock launches (L = padded stage length in rows)"""
    C = cfg["upsample_initial_channel"] >> len(cfg["upsample_rates"])
    nk = len(cfg["resblock_kernel_sizes"])
    out = {}
    for j, (k, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
        wav = j == nk - 1 and nk >= 2
        out[f"rbn<{C}> k={k} d={tuple(dils)}{' +post' if wav else ''}"] = tile_rows(C, k, dils, B, L, wav, cus)
    return out
