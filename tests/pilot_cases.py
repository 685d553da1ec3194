"""Inputs of the pilot-stage edge tests (tests/test_pilot_cases_host.py on the CPU, tests/test_gpu_pilot_edges.py on the GPU):
a geometry table that reaches every lane-group size of pilot_track_kernel, rows with a PLANTED rotation phi + tau k large enough
for the range reduction and the DC skip to matter, rows whose pilot sum is not usable, and a float32 NumPy emulation of the
contract's operation order.  NumPy only, deterministic."""
import numpy as np

import pilot_ref as pr
from oracle import ofdm_oracle as orc

BPS = {"QPSK": 2, "16QAM": 4, "64QAM": 6}
MODS = ("QPSK", "16QAM", "64QAM")
PVS = (0.6 - 0.8j, -1 + 1j, 1j)                                       # the second is not of unit magnitude
THETA_CAP = 2.4                                                       # radians at the outermost pilot: theta must not wrap


# ------------------------------------------------------------------------------------------ the kernel's work split, restated
def group_log2(Kd):
    """pilot_group_log2 of csrc/ofdm_launch.hpp: a row of Kd data entries belongs to 2^g lanes"""
    g = 1
    while g < 6 and (1 << g) < (Kd + 1) // 2:
        g += 1
    return g


def rows_per_group(K, g_log2):
    """pilot_rows_per_group of csrc/ofdm_launch.hpp"""
    return max(1, 4096 // (K * 8 * (64 >> g_log2)))


def comb(K, per_side, step=None):
    """symmetric comb: +-step, +-2 step, .. (step: the widest that fits per_side + 1 steps into half the band)"""
    step = step or (K // 2) // (per_side + 1)
    return [s * step * m for m in range(1, per_side + 1) for s in (-1, 1)]


def all_but(K, drop=()):
    h = K // 2
    return [k for k in list(range(-h, 0)) + list(range(1, h + 1)) if k not in drop]


#        nfft  cp   K     pilot locations                       Kd'   G   what the row is there for
GEOMS = [(64, 16, 2, [1]),                                     # 1    2   one pilot: CPE only; a single output, a single byte of bits
         (64, 16, 4, [-2, 2]),                                 # 2    2
         (64, 16, 6, [-1, 1]),                                 # 4    2   inner pilots: the band edge passes pi
         (64, 16, 8, [-3, 3]),                                 # 6    4   16-QAM: Kd' % 4 == 2
         (64, 16, 8, [-1, 1]),                                 # 6    4   inner pilots
         (64, 16, 16, [-5, 5]),                                # 14   8   Kd' % 4 == 2
         (64, 16, 16, [-2, 2]),                                # 14   8   inner pilots
         (64, 16, 28, [-9, -3, 3, 9]),                         # 24   16
         (64, 16, 28, [-5, -2, 2, 5]),                         # 24   16  inner pilots
         (64, 16, 60, [-21, -7, 7, 21]),                       # 56   32
         (64, 16, 60, [-9, -3, 3, 9]),                         # 56   32  inner pilots
         (128, 10, 100, comb(100, 4)),                         # 92   64  5 rows per group
         (256, 18, 152, comb(152, 4)),                         # 144  64  3 rows per group
         (512, 36, 300, comb(300, 6)),                         # 288  64  1 row per group, two load batches
         (1024, 72, 600, comb(600, 8)),                        # 584  64  three load batches
         (1024, 72, 600, comb(600, 8, 16)),                    # 584  64  pilots within +-K/4: the band edge passes pi
         (2048, 144, 1200, comb(1200, 100, 6)),                # 1000 64  200 pilots: four pilot trips, the last of 8
         (64, 16, 60, all_but(60)),                            # 0    2   no data: cpe and cfo only, 30 pilot trips
         (64, 16, 60, all_but(60, (30,)))]                     # 1    2   one data entry at the band edge; asymmetric pilots


def geom_id(g):
    nfft, cp, K, locs = g
    return "N%d-K%d-p%d_%d" % (nfft, K, len(locs), max(abs(x) for x in locs))


BY_ID = {geom_id(g): g for g in GEOMS}


def describe(g):
    nfft, cp, K, locs = g
    Kd = K - len(locs)
    gl = group_log2(Kd)
    return dict(nfft=nfft, cp=cp, K=K, n_pilots=len(locs), Kd=Kd, g_log2=gl, G=1 << gl, rows_per_group=rows_per_group(K, gl),
                pilot_trips=-(-len(locs) // (1 << gl)), last_trip=(len(locs) - 1) % (1 << gl) + 1,
                load_batches=-(-((Kd + 1) // 2) // (2 << gl)), symmetric=sorted(locs) == sorted(-x for x in locs))


def offsets(K):
    h = K // 2
    return np.array(list(range(-h, 0)) + list(range(1, h + 1)), dtype=np.float64)


def tau_max(K, locations):
    """The largest slope (radians per bin) planted on a geometry: |tau| max|k_p| <= THETA_CAP, lowered until the pilot set can
    carry it -- for every slope up to it the noise-free pilot sum keeps a quarter of its length (two pilots at +-k lose all of it
    at tau k = pi/2) and every theta_p stays 0.4 rad inside (-pi, pi).  0 with fewer than two pilots."""
    pk = pr.layout(K, locations)[1].astype(np.float64)
    if len(pk) < 2:
        return 0.0
    best = 0.0
    for t in np.linspace(0.0, THETA_CAP / np.max(np.abs(pk)), 241)[1:]:
        w = np.exp(1j * t * pk)
        U = w.sum()
        if abs(U) < 0.25 * len(pk) or np.max(np.abs(np.angle(w * np.conj(U) / abs(U)))) > np.pi - 0.4:
            break
        best = float(t)
    return best


# ------------------------------------------------------------------------------------------ planted rows
def planted_rows(geom, mod, pilot_value, rows, seed, mode=pr.CPE_SLOPE):
    """-> (z complex64 [rows][K], sym complex128 [rows][Kd'], bits uint8 [rows][Kd' bps], phi [rows], tau [rows]).
    Pilot entries pilot_value, data entries exact points of orc.map_bits, the whole row times e^{j(phi + tau k)}, k the signed
    offset of the list index.  phi uniform in (-pi, pi); tau uniform in +-tau_max(geom), rows 0 and 1 AT +-tau_max so that the
    largest phase of a case does not hang on the draw.  In CPE mode (the stage cannot remove a slope) and with one pilot: tau = 0."""
    nfft, cp, K, locs = geom
    pidx, pk, didx, dk = pr.layout(K, locs)
    Kd, bps = len(didx), BPS[mod]
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (rows, Kd * bps)).astype(np.uint8)
    sym = orc.map_bits(bits.ravel(), mod).reshape(rows, Kd) if Kd else np.zeros((rows, 0), np.complex128)
    phi = rng.uniform(-np.pi, np.pi, rows)
    tau = rng.uniform(-1.0, 1.0, rows)
    tau[:2] = [1.0, -1.0][:rows]
    tau = tau * (tau_max(K, locs) if mode == pr.CPE_SLOPE else 0.0)
    z = np.zeros((rows, K), np.complex128)
    z[:, pidx] = complex(pilot_value)
    z[:, didx] = sym
    z = z * np.exp(1j * (phi[:, None] + tau[:, None] * offsets(K)[None, :]))
    return z.astype(np.complex64), sym, bits, phi, tau


# ------------------------------------------------------------------------------------------ rows without a usable U
KINDS = ("nan", "+inf", "-inf", "cancel", "1e25", "1e-30")


def random_rows(rng, n, K, locs, pilot_value=1.0 + 0j, phase_step=None):
    """rows that look like equalised symbols (as _rows of tests/test_gpu_pilot_frames.py): unit-power data, pilots near
    pilot_value times a common rotation per row -- a random one, or phase_step radians further per row (a planted carrier
    offset: the cfo sum is then coherent and its argument well conditioned)."""
    z = (rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))) / np.sqrt(2)
    pidx = pr.layout(K, locs)[0]
    ph = rng.uniform(-np.pi, np.pi, n) if phase_step is None else rng.uniform(-np.pi, np.pi) + phase_step * np.arange(n)
    z[:, pidx] = complex(pilot_value) * np.exp(1j * ph)[:, None] * (
        1 + 0.05 * (rng.standard_normal((n, len(locs))) + 1j * rng.standard_normal((n, len(locs)))))
    return z.astype(np.complex64)


def spoil(z, row, pidx, kind, rng):
    """overwrite the PILOT entries of z[row] so that its pilot sum is not usable"""
    n = len(pidx)
    if kind == "nan":
        z[row, pidx] = complex(np.nan, np.nan)
    elif kind == "+inf":
        z[row, pidx[n // 2]] = complex(np.inf, 0.25)
    elif kind == "-inf":
        z[row, pidx[n // 2]] = complex(0.25, -np.inf)
    elif kind == "cancel":                                            # (+a, -a) neighbours: every partial sum of a pair is exactly 0
        a = np.exp(1j * rng.uniform(-np.pi, np.pi, n // 2)).astype(np.complex64)
        v = np.zeros(n, np.complex64)
        v[n % 2::2] = a
        v[n % 2 + 1::2] = -a
        z[row, pidx] = v
    elif kind == "1e25":
        z[row, pidx] = 1e25
    elif kind == "1e-30":
        z[row, pidx] = 1e-30
    else:
        raise ValueError(kind)


def unusable_choice(geom, rows):
    """the rows unusable_rows spoils: the first, the last, s = 63, 64, 65 of a segment of 130 rows and more, the middle row of a
    lane group's walk (rows_per_group > 1) or a row between usable neighbours of its wave, then every seventh until all KINDS
    are used"""
    d = describe(geom)
    rpg = d["rows_per_group"]
    rows_ = [0, rows - 1] + ([63, 64, 65] if rows >= 130 else [])
    rows_.append(2 * rpg + rpg // 2 if rpg > 1 else 3)
    s = 10
    while len(set(rows_)) < len(KINDS):
        if s not in rows_:
            rows_.append(s)
        s += 7
    out = sorted(set(rows_))
    assert out[-1] == rows - 1 and len(out) >= len(KINDS), "segment too short"
    return out


def unusable_rows(geom, rows, seed, pilot_value=1.0 + 0j, phase_step=None, chosen=None):
    """-> (z complex64 [rows][K], plain complex64 [rows][K], kinds {row: kind}): `plain` are ordinary rows, z the same rows with
    the PILOT entries of the chosen rows overwritten (KINDS in turn, starting at `seed`); data entries stay finite."""
    nfft, cp, K, locs = geom
    rng = np.random.default_rng(seed)
    plain = random_rows(rng, rows, K, locs, pilot_value, phase_step)
    z = plain.copy()
    pidx = pr.layout(K, locs)[0]
    kinds = {}
    for i, r in enumerate(unusable_choice(geom, rows) if chosen is None else chosen):
        kinds[r] = KINDS[(i + seed) % len(KINDS)]
        spoil(z, r, pidx, kinds[r], rng)
    return z, plain, kinds


# ------------------------------------------------------------------------------------------ the contract in float32
def _f(x):
    return np.asarray(x, dtype=np.float32)


def _cmul(a, b):
    """(ar, ai) * (br, bi) as the kernels' cmul: re = fma(ai, -bi, ar br), im = fma(ar, bi, ai br)"""
    ar, ai = a
    br, bi = b
    d = np.float64
    return (_f(ai.astype(d) * -bi.astype(d) + _f(ar * br).astype(d)), _f(ar.astype(d) * bi.astype(d) + _f(ai * br).astype(d)))


def emulate_f32(z, locations, pilot_value, mode):
    """The stage with every operation of the contract rounded to float32 in the kernel's order (U and the theta sums in
    ascending p, c = conj(U) / sqrt(|U|^2), the phase in revolutions reduced by rint, then sin / cos -- taken exactly here, so
    the hardware's sin / cos error is NOT in the figure).  z [rows][K] complex64 with usable rows -> dict(data, cpe, slope)."""
    z = np.asarray(z, np.complex64)
    rows, K = z.shape
    pidx, pk, didx, dk = pr.layout(K, locations)
    n = len(pidx)
    with np.errstate(all="ignore"):
        pc = (_f(np.full(rows, np.real(pilot_value))), _f(np.full(rows, -np.imag(pilot_value))))
        w = [_cmul((_f(z[:, p].real), _f(z[:, p].imag)), pc) for p in pidx]
        ur, ui = _f(np.zeros(rows)), _f(np.zeros(rows))
        for wr, wi in w:
            ur, ui = _f(ur + wr), _f(ui + wi)
        inv = _f(np.float32(1.0) / np.sqrt(_f(ur * ur + ui * ui)))
        c = (_f(ur * inv), _f(-ui * inv))
        out = dict(cpe=(ur * inv).astype(np.complex64) + 1j * _f(ui * inv), slope=_f(np.zeros(rows)))
        zr, zi = _f(z[:, didx].real), _f(z[:, didx].imag)
        if mode != pr.CPE_SLOPE:
            dr, di = _cmul((c[0][:, None] + 0 * zr, c[1][:, None] + 0 * zr), (zr, zi))
            out["data"] = dr + 1j * di
            return out
        kbar = np.float32(pk.mean())
        inv_skk = np.float32(1.0 / ((pk - pk.mean()) ** 2).sum())
        st, skt = _f(np.zeros(rows)), _f(np.zeros(rows))
        for (wr, wi), k in zip(w, pk):
            tr, ti = _cmul((wr, wi), c)
            th = _f(np.arctan2(ti, tr))
            st, skt = _f(st + th), _f(skt + _f(_f(np.float32(k) - kbar) * th))
        tau = _f(skt * inv_skk)
        delta = _f(_f(st / np.float32(n)) - _f(tau * kbar))
        rev = _f(_f(delta[:, None] + _f(tau[:, None] * _f(dk)[None, :])) * np.float32(0.15915494309189535))
        rev = _f(rev - np.rint(rev))
        ang = 2 * np.pi * rev.astype(np.float64)
        rot = _cmul((c[0][:, None] + 0 * rev, c[1][:, None] + 0 * rev), (_f(np.cos(ang)), _f(-np.sin(ang))))
        dr, di = _cmul(rot, (zr, zi))
        out.update(data=dr + 1j * di, slope=tau)
    return out


# ------------------------------------------------------------------------------------------ end to end: a one-sample timing error
#       nfft cp  K    pilots          constellation  eps    noise   (noise: the level test_gpu_pilot_frames.py uses for it)
E2E = [(128, 10, 100, comb(100, 4), "16QAM", 0.005, 0.005),
       (256, 18, 152, comb(152, 4), "QPSK", 0.01, 0.02)]
E2E_PV = 0.6 - 0.8j
E2E_SYM, E2E_FRAMES = 16, 2


def e2e_frames(case):
    """-> (iq complex64 [2][frame_len], bits uint8 [2][12 Kd' bps]): frames of 16 symbols whose 12 data rows carry a random
    phase and a slope that runs from minus to plus a one-sample timing error (2 pi / N per bin)"""
    nfft, cp, K, locs, mod, eps, noise = case
    n_data = E2E_SYM // 4 * 3
    fr = []
    for f in range(E2E_FRAMES):
        rng = np.random.default_rng(100 + f)
        slope = np.linspace(-1.0, 1.0, n_data)[::1 if f == 0 else -1] * 2 * np.pi / nfft
        fr.append(pr.make_frame(nfft, cp, K, locs, mod, E2E_SYM, eps, noise, seed=11 + f, pilot_value=E2E_PV,
                                row_phase=rng.uniform(-np.pi, np.pi, n_data), row_slope=slope))
    return np.stack([x for x, _ in fr]).astype(np.complex64), np.stack([b for _, b in fr])
