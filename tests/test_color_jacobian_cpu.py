"""The colour Jacobian of the SH evaluation (sgr_math.h: sgr_sh_color_jacobian, sgr_jac_times_drgb) on the host, no GPU.

The preprocess stores J = d rgb / d dir and the per-Gaussian backward forms dL/ddir = J . dL/dRGB; the row-reading backward
contracts the SH row with dL/dRGB first (t[k]) and then applies the same polynomial (sgr_sh_dir_backward).  Both are float32
evaluations of ONE polynomial in another association.  A small stand-alone host program evaluates, for 10 000 random
(dir, sh, dRGB) per SH degree 0..3: the J form, the t form, and a float64 evaluation (the reference's per-channel form,
backward.cu:46-136, written out in the program) on the same float32 inputs -- the truth.

Gate (set by the issue): the J form's error is within 2 x the t form's own error on the same inputs.  "Error" is taken
over the whole sample, as the root mean square and as the maximum of |value - truth| over all samples and components: a
per-sample ratio is meaningless (either form hits the truth exactly on many samples).  The measured ratios are printed."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "street_gaussians_amd", "csrc")

PROGRAM = r"""
#include "sgr_math.h"
#include <cstdint>
#include <cstdio>

static uint64_t s = 0x9E3779B97F4A7C15ull;
static double uni() {  // xorshift64*: uniform in (-1, 1)
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (double)((s * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// float64, the reference's association: dRGB/dx, dRGB/dy, dRGB/dz per channel, then the dot with dL/dRGB
static void truth(int deg, const float* dir, const float* sh, const float* dRGB, double* out) {
    const double x = dir[0], y = dir[1], z = dir[2];
    const double C1 = SGR_SH_C1, C2[5] = {SGR_SH_C2_0, SGR_SH_C2_1, SGR_SH_C2_2, SGR_SH_C2_3, SGR_SH_C2_4};
    const double C3[7] = {SGR_SH_C3_0, SGR_SH_C3_1, SGR_SH_C3_2, SGR_SH_C3_3, SGR_SH_C3_4, SGR_SH_C3_5, SGR_SH_C3_6};
    out[0] = out[1] = out[2] = 0.0;
    for (int c = 0; c < 3; c++) {
        auto h = [&](int k) { return (double)sh[3 * k + c]; };
        double dx = 0, dy = 0, dz = 0;
        if (deg > 0) {
            dx = -C1 * h(3); dy = -C1 * h(1); dz = C1 * h(2);
            if (deg > 1) {
                const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                dx += C2[0] * y * h(4) + C2[2] * 2.0 * -x * h(6) + C2[3] * z * h(7) + C2[4] * 2.0 * x * h(8);
                dy += C2[0] * x * h(4) + C2[1] * z * h(5) + C2[2] * 2.0 * -y * h(6) + C2[4] * 2.0 * -y * h(8);
                dz += C2[1] * y * h(5) + C2[2] * 2.0 * 2.0 * z * h(6) + C2[3] * x * h(7);
                if (deg > 2) {
                    dx += C3[0] * h(9) * 3.0 * 2.0 * xy + C3[1] * h(10) * yz + C3[2] * h(11) * -2.0 * xy + C3[3] * h(12) * -3.0 * 2.0 * xz +
                          C3[4] * h(13) * (-3.0 * xx + 4.0 * zz - yy) + C3[5] * h(14) * 2.0 * xz + C3[6] * h(15) * 3.0 * (xx - yy);
                    dy += C3[0] * h(9) * 3.0 * (xx - yy) + C3[1] * h(10) * xz + C3[2] * h(11) * (-3.0 * yy + 4.0 * zz - xx) +
                          C3[3] * h(12) * -3.0 * 2.0 * yz + C3[4] * h(13) * -2.0 * xy + C3[5] * h(14) * -2.0 * yz + C3[6] * h(15) * -3.0 * 2.0 * xy;
                    dz += C3[1] * h(10) * xy + C3[2] * h(11) * 4.0 * 2.0 * yz + C3[3] * h(12) * 3.0 * (2.0 * zz - xx - yy) +
                          C3[4] * h(13) * 4.0 * 2.0 * xz + C3[5] * h(14) * (xx - yy);
                }
            }
        }
        out[0] += dx * dRGB[c]; out[1] += dy * dRGB[c]; out[2] += dz * dRGB[c];
    }
}

int main() {
    const int N = 10000;
    for (int deg = 0; deg <= 3; deg++) {
        double sj = 0, st = 0, mj = 0, mt = 0;
        for (int n = 0; n < N; n++) {
            double d[3] = {uni(), uni(), uni()};
            if (n % 100 == 0) { d[0] = 1.0; d[1] *= 1e-3; d[2] *= 1e-3; }  // near a coordinate axis
            const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const float dir[3] = {(float)(d[0] / len), (float)(d[1] / len), (float)(d[2] / len)};
            float sh[48], dRGB[3];
            for (int e = 0; e < 48; e++) sh[e] = (float)(0.3 * uni() * (e < 3 ? 1.0 : 0.3));
            for (int c = 0; c < 3; c++) dRGB[c] = (n % 7 == 0 && c == n % 3) ? 0.f : (float)uni();  // some clamped channels
            float J[9], vj[3], t[16], vt[3];
            sgr_sh_color_jacobian(deg, dir[0], dir[1], dir[2], sh, J);
            sgr_jac_times_drgb(J, dRGB, vj);
            for (int k = 0; k < 16; k++) t[k] = k < (deg + 1) * (deg + 1) ? sh[3 * k] * dRGB[0] + sh[3 * k + 1] * dRGB[1] + sh[3 * k + 2] * dRGB[2] : 0.f;
            sgr_sh_dir_backward(deg, dir[0], dir[1], dir[2], t, vt);
            double tr[3];
            truth(deg, dir, sh, dRGB, tr);
            for (int a = 0; a < 3; a++) {
                const double ej = fabs((double)vj[a] - tr[a]), et = fabs((double)vt[a] - tr[a]);
                sj += ej * ej; st += et * et;
                if (ej > mj) mj = ej;
                if (et > mt) mt = et;
            }
        }
        printf("deg %d rms_j %.9e rms_t %.9e max_j %.9e max_t %.9e\n", deg, sqrt(sj / (3.0 * N)), sqrt(st / (3.0 * N)), mj, mt);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def measured(tmp_path_factory):
    d = tmp_path_factory.mktemp("color_jacobian")
    src, exe = str(d / "jac_host.hip"), str(d / "jac_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I", CSRC, src, "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        w = line.split()
        rows[int(w[1])] = {w[i]: float(w[i + 1]) for i in range(2, len(w), 2)}
    assert sorted(rows) == [0, 1, 2, 3], out
    return rows


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_j_form_is_as_close_to_float64_as_the_t_form(measured, deg):
    r = measured[deg]
    ratio = {k: (r[k + "_j"] / r[k + "_t"] if r[k + "_t"] > 0 else float("nan")) for k in ("rms", "max")}
    print(f"degree {deg}: J form / t form error ratio: rms {ratio['rms']:.3f} (J {r['rms_j']:.3e}, t {r['rms_t']:.3e}), "
          f"max {ratio['max']:.3f} (J {r['max_j']:.3e}, t {r['max_t']:.3e})")
    if deg == 0:  # no direction dependence: both forms give exactly zero
        assert r["max_j"] == 0.0 and r["max_t"] == 0.0
        return
    assert r["rms_t"] > 0 and r["rms_j"] > 0  # the sample exercises both forms
    assert r["rms_j"] <= 2.0 * r["rms_t"], (deg, r)
    assert r["max_j"] <= 2.0 * r["max_t"], (deg, r)
