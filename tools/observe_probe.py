#!/usr/bin/env python3
"""Times K16 (rjp_uv_tracks, rjp_vis_noise: one launch each) against torch routes to the same
products that stay on the device, on the same buffers, in ONE process:

    python tools/observe_probe.py [--point vla|big|all] [--rounds N] [--out FILE.json]

The torch routes: for the tracks the three rotation rows per integration from `torch.sin` /
`torch.cos` of the hour angles and ONE `einsum('itj,bj->itb')` with the baseline vectors (no
elevation flags: the K16 side is timed without them too, and once more with them); for the noise
`torch.randn` of the stack's shape and the scaled add `V + sigma[:, None, None] * s[None, :, None] * g`
(torch's own Philox stream: other numbers, and no (seed, map, visibility) addressing -- a chunked
call does not reproduce the whole).  No parent kernel exists: torch is the yardstick.
vla = the 27-antenna list of tests/golden at t_obs / t_int = 720 integrations (252 720
visibilities), noise on 8 maps; big = 244 antennas scattered over 16 km at 720 integrations
(21 345 120 visibilities), noise on 1 map.  Every shape is warmed up once; then the routes are
timed with device events in alternating rounds; minimum, median and maximum of each are reported
with the ratio of the medians, the worst case for K16 (its slowest round against torch's fastest)
and the bytes each K16 launch moves per visibility."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "antenna_configs", "vla.a.cfg")
N_T = 720
POINTS = {"vla": (27, 8), "big": (244, 1)}        # antennas, maps of the noise stack


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def array_of(n_ant):
    if n_ant == 27:
        xyz = E.read_antenna_config(FIXTURE).xyz
    else:
        rng = np.random.default_rng(n_ant)
        lat, lon = np.radians(-23.02), np.radians(-67.75)
        east = np.array([-np.sin(lon), np.cos(lon), 0.])
        north = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
        up = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
        r, th = 8000. * np.sqrt(rng.uniform(0, 1, n_ant)), rng.uniform(0, 2 * np.pi, n_ant)
        xyz = 6.383e6 * up + (r * np.cos(th))[:, None] * east + (r * np.sin(th))[:, None] * north
    return xyz, E.geodetic(xyz)


def torch_tracks(gha, b, sd, cd):
    G = 2.0 * np.pi * gha
    s, c, z = torch.sin(G), torch.cos(G), torch.zeros_like(G)
    rot = torch.stack([torch.stack([s, c, z], dim=1),
                       torch.stack([-sd * c, sd * s, cd + z], dim=1),
                       torch.stack([cd * c, -cd * s, sd + z], dim=1)], dim=0)          # [3, T, 3]
    uvw = torch.einsum('itj,bj->itb', rot, b)
    return uvw[0], uvw[1], uvw[2]


def probe(eng, name, rounds):
    n_ant, M = POINTS[name]
    xyz, geo = array_of(n_ant)
    dec = np.radians(18.0 if n_ant == 27 else -30.0)
    sd, cd = float(np.sin(dec)), float(np.cos(dec))
    ha = (np.arange(N_T) + 0.5 - 0.5 * N_T) * 10. / E.SIDEREAL_DAY_S
    gha = ha - geo.lon0_deg / 360.
    i, j = np.triu_indices(n_ant, 1)
    B = len(i)
    K = N_T * B
    d_gha = torch.from_numpy(gha).to(eng.device)
    d_b = torch.from_numpy(xyz[j] - xyz[i]).to(eng.device)

    routes = {"k16_tracks": lambda: eng.uv_tracks(xyz, gha, dec),
              "k16_tracks_flags": lambda: eng.uv_tracks(xyz, gha, dec, up=geo.up, min_el_rad=0.2),
              "torch_tracks": lambda: torch_tracks(d_gha, d_b, sd, cd)}
    g = torch.Generator(device=eng.device)
    g.manual_seed(20240518)
    V = torch.randn(M, K, 2, dtype=torch.float64, device=eng.device, generator=g)
    s = 0.5 + torch.rand(K, dtype=torch.float64, device=eng.device, generator=g)
    sig_h = 0.5 + 0.1 * np.arange(M)
    sig = torch.from_numpy(sig_h).to(eng.device)

    def torch_noise():
        return torch.add(V, sig[:, None, None] * s[None, :, None] * torch.randn(V.shape, dtype=torch.float64,
                                                                                 device=eng.device, generator=g))
    routes["k16_noise"] = lambda: eng.vis_noise(V, sig_h, seed=7, s=s)
    routes["torch_noise"] = torch_noise
    # warm-up of every shape, and the agreement of the two routes where they compute the same thing
    a = routes["k16_tracks"]()
    b = routes["torch_tracks"]()
    scale = float(d_b.abs().sum(dim=1).max().item())
    diff = max(float((x - y).abs().max().item()) for x, y in zip(a, b)) / scale
    flagged = float(torch.isnan(routes["k16_tracks_flags"]()[0]).double().mean().item())
    noisy = routes["k16_noise"]()
    spread = float(((noisy - V)[0, :, 0] / (sig_h[0] * s)).std().item())
    routes["torch_noise"]()
    del a, b, noisy
    eng.synchronize()
    t = {n: [] for n in routes}
    for _ in range(rounds):                                   # alternating rounds
        for n, fn in routes.items():
            ms, res = timed(fn)
            t[n].append(ms)
            del res
    med = lambda x: float(np.median(x))
    rec = {"point": name, "antennas": n_ant, "baselines": B, "integrations": N_T, "visibilities": K,
           "noise_maps": M, "rounds": rounds,
           "tracks_bytes_per_visibility": 24, "noise_bytes_per_visibility_and_map": 32 + 8. / M,
           "tracks_max_difference_over_b": diff, "flagged_fraction": flagged, "noise_std_over_sigma": spread,
           "torch_over_k16_tracks_median": med(t["torch_tracks"]) / med(t["k16_tracks"]),
           "torch_over_k16_tracks_worst_case": min(t["torch_tracks"]) / max(t["k16_tracks"]),
           "torch_over_k16_noise_median": med(t["torch_noise"]) / med(t["k16_noise"]),
           "torch_over_k16_noise_worst_case": min(t["torch_noise"]) / max(t["k16_noise"]),
           "k16_tracks_gb_per_s": 24. * K / (med(t["k16_tracks"]) * 1e6),
           "k16_noise_gb_per_s": (32. * M + 8.) * K / (med(t["k16_noise"]) * 1e6)}
    for n in routes:
        rec["ms_" + n] = [min(t[n]), med(t[n]), max(t[n])]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs = []
    for name in (tuple(POINTS) if args.point == "all" else (args.point,)):
        torch.cuda.empty_cache()
        recs.append(probe(eng, name, args.rounds))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
