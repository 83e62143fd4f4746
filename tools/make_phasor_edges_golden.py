"""Writes tests/golden/phasor_edges_mp.npz: the phasance columns of tests/matrices_edges_util.phasor_cases() evaluated with
mpmath at 40 digits on the float64 inputs exactly as given (phasance.py:19-52, 62-82, 108-144), rounded to float64 once at the
end, next to the inputs themselves.  The GPU test reads the file; the CPU test regenerates it where mpmath is installed.

  zm [nf][nnu]  = F(b) - F(a),  F(nu) = sqrt(pi)/2 / eps * exp(nu_m L + L^2 / (4 eps^2)) * erf(eps (nu - nu_m) - L / (2 eps)),
                  L = ln(j omega) = ln(2 pi f) + j pi/2,  (a, b) = (min(0, sgn nu_m), max(0, sgn nu_m))
  vlay [k][nt][nnu] = size_k (G(b) - G(a)) for t > t_k, else 0,
                  G(nu) = sqrt(pi)/2 / eps * dt^-nu_m / Gamma(1 - nu_m) * exp(ln(dt)^2 / (4 eps^2)) * erf(eps (nu - nu_m) + ln(dt) / (2 eps))
  vm = sum over k

    python tools/make_phasor_edges_golden.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def evaluate(case, digits=40):
    import mpmath as mp
    mp.mp.dps = digits
    eps = mp.mpf(float(case["eps"]))
    half_rt_pi = mp.sqrt(mp.pi) / 2

    def limits(num):
        sg = mp.sign(num)
        return min(mp.mpf(0), sg), max(mp.mpf(0), sg)

    nf, nnu, nt = len(case["freq"]), len(case["nu"]), len(case["times"])
    zm = np.zeros((nf, nnu), dtype=complex)
    for r, f in enumerate(case["freq"]):
        L = mp.log(2 * mp.pi * mp.mpf(float(f))) + 1j * mp.pi / 2
        for c, num in enumerate(case["nu"]):
            num = mp.mpf(float(num))
            a, b = limits(num)
            pre = half_rt_pi / eps * mp.exp(num * L + L * L / (4 * eps * eps))
            val = pre * (mp.erf(eps * (b - num) - L / (2 * eps)) - mp.erf(eps * (a - num) - L / (2 * eps)))
            zm[r, c] = complex(val)
    steps = list(zip(case["step_times"], case["step_sizes"]))
    vlay = np.zeros((len(steps), nt, nnu))
    vm = np.zeros((nt, nnu))
    for r, t in enumerate(case["times"]):
        for c, num in enumerate(case["nu"]):
            num = mp.mpf(float(num))
            a, b = limits(num)
            total = mp.mpf(0)
            for k, (st, sa) in enumerate(steps):
                if not float(t) > float(st):
                    continue
                ldt = mp.log(mp.mpf(float(t)) - mp.mpf(float(st)))
                pre = half_rt_pi / eps * mp.exp(-num * ldt) * mp.rgamma(1 - num) * mp.exp(ldt * ldt / (4 * eps * eps))
                val = mp.mpf(float(sa)) * pre * (mp.erf(eps * (b - num) + ldt / (2 * eps)) - mp.erf(eps * (a - num) + ldt / (2 * eps)))
                vlay[k, r, c] = float(val)
                total += val
            vm[r, c] = float(total)
    return zm, vm, vlay


def build():
    import matrices_edges_util as mu
    out = {}
    for name, case in mu.phasor_cases().items():
        zm, vm, vlay = evaluate(case)
        for key in ("freq", "nu", "times", "step_times", "step_sizes"):
            out[f"{name}.{key}"] = np.asarray(case[key], dtype=float)
        out[f"{name}.eps"] = np.float64(case["eps"])
        out[f"{name}.zm_re"], out[f"{name}.zm_im"] = zm.real.copy(), zm.imag.copy()
        out[f"{name}.vm"], out[f"{name}.vlay"] = vm, vlay
    return out


if __name__ == "__main__":
    import matrices_edges_util as mu
    path = sys.argv[1] if len(sys.argv) > 1 else mu.PHASOR_GOLDEN
    data = build()
    np.savez_compressed(path, **data)
    print(f"{path}: {len(data)} arrays, {sum(v.size for v in data.values())} numbers, {os.path.getsize(path)} bytes")
