"""GPU - emulator bounds of tests/test_hifigan_v2_gpu.py for the isolating C = 16 / C = 8 generators and the full V2 generator: per-sample max,
largest 256-sample windowed RMS, global RMS.  They are vocoder_emul.BOUNDS — the new kernel rounds where rblock rounds and differs from the
emulator by fp32 summation order only — except the bf16 per-sample maximum of the isolating generators: at 3.1e-3 the smallest planted defect
of tests/test_hifigan_v2_cpu.py (the last convolution's farthest halo row of one tile missing: 1.4e-3 at C = 8) would hide inside it, so it is
1.3e-3 here = 3 x the largest per-sample difference between the float64 and the float32 evaluation of the SAME bf16 rounding points on these
generators (4.4e-4, the 9000-frame mel of test_narrow_bounds_against_the_emulators_own_noise: what a change of summation order alone does).
Never above vocoder_emul.BOUNDS (test_narrow_bounds_do_not_exceed_resblock1s)."""
from vocoder_emul import BOUNDS

NARROW_BOUNDS = {
    "f16": dict(BOUNDS["f16"]),
    "bf16": {**BOUNDS["bf16"], "max": 1.3e-3},
    "full_f16": dict(BOUNDS["full_f16"]),
    "full_bf16": dict(BOUNDS["full_bf16"]),
}
