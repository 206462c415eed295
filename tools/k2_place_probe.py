#!/usr/bin/env python3
"""What the placement of the two product cubes does to K2 (ff_maps_acc_kernel), per build of
librjprt: `tau` and `flux` of cfg4's map stage (262144 pixels x 256 channels, one epoch, with the
totals) are carved out of ONE buffer, flux at the cube size + 0, 256 B, 4 KiB, 64 KiB and
1 MiB + 4 KiB behind tau, and every build stores into the SAME bytes in ONE process, alternating,
`--rounds` x `--reps` launches per offset between HIP events.  A second sweep follows after
~40 GB were allocated in 1 GiB chunks and two of every three handed back to the driver (the buffer
then lies where the driver puts it among the chunks still held), a third takes two separate allocations, what engine.ff_maps does by default.  At the first
offset the cubes and totals of every build are compared bit for bit with the first named build's.

    python tools/k2_place_probe.py --out profiles/k2_placement.json \\
        parent=rajepy_amd/librjprt_parent.so kouter=rajepy_amd/librjprt_kouter.so

(the default build takes part as "new"; -DRJP_K2_CHOUTER=0 builds the pixel-group-outer order,
see ff_scan.hip)
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from rajepy_amd import _lib, engine as E  # noqa: E402

NPIX, NCHAN = 512 * 512, 256
OFFSETS = (0, 256, 4096, 65536, (1 << 20) + 4096)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="name=path of further builds; the first is the yardstick")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--churn-gb", type=int, default=40)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    builds = []
    for spec in args.libs:
        name, path = spec.split("=", 1)
        lib = C.CDLL(os.path.abspath(path))
        for fn_name, (res, argt) in _lib.SIGNATURES.items():
            fn = getattr(lib, fn_name)
            fn.restype, fn.argtypes = res, argt
        assert lib.rjp_version() == _lib.RJP_VERSION
        ctx = C.c_void_p()
        assert lib.rjp_ctx_create(0, C.byref(ctx)) == 0
        builds.append((name, lib, ctx))
    builds.append(("new", eng.lib, eng.ctx))
    rng = np.random.default_rng(10)
    A = rng.uniform(1e-3, 3e3, (1, NPIX)) * 10.0 ** rng.uniform(-8, 2, (1, NPIX))
    T = rng.uniform(5e3, 2e4, NPIX)
    T[rng.random(NPIX) < 0.01] = np.nan
    A[:, np.isnan(T)] = 0.0
    dA, dT = torch.from_numpy(A).to(eng.device), torch.from_numpy(T).to(eng.device)
    ctau = _lib.dbl_array(10.0 ** rng.uniform(-6, 1, NCHAN))
    cflux = _lib.dbl_array(10.0 ** rng.uniform(-12, -8, NCHAN))
    cube = NPIX * NCHAN * 8
    work = torch.empty(int(eng.lib.rjp_ff_maps_workspace(NPIX, 1, NCHAN)), dtype=torch.uint8,
                       device=eng.device)
    ftot = {name: eng._f64(1, NCHAN) for name, _, _ in builds}

    def launch(name, lib, ctx, tau, flux):
        st = lib.rjp_ff_maps(ctx, dA.data_ptr(), dT.data_ptr(), NPIX, 1, ctau, cflux, NCHAN,
                             tau.data_ptr(), flux.data_ptr(), ftot[name].data_ptr(),
                             work.data_ptr(), work.numel(), eng._stream())
        assert st == 0, (name, lib.rjp_last_error(ctx))

    def timed(name, lib, ctx, tau, flux, reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            launch(name, lib, ctx, tau, flux)
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / reps          # microseconds per launch

    def sweep(places):
        """places: [(label, tau, flux)] -> {label: {build: {us: [...], ...}}}"""
        rows = {lab: {name: {"us": []} for name, _, _ in builds} for lab, _, _ in places}
        for lab, tau, flux in places:
            for b in builds:
                timed(*b, tau, flux, 2)
        for _ in range(args.rounds):
            for lab, tau, flux in places:
                for b in builds:
                    rows[lab][b[0]]["us"].append(timed(*b, tau, flux, args.reps))
        for lab in rows:
            for name in rows[lab]:
                us = np.array(rows[lab][name]["us"])
                rows[lab][name].update(us_mean=float(us.mean()), us_min=float(us.min()),
                                       us_max=float(us.max()))
        return rows

    def carve(buf):
        base = (-buf.data_ptr()) % 4096                         # tau on a 4 KiB boundary
        out = []
        for off in OFFSETS:
            tau = buf[base:base + cube].view(torch.float64)
            flux = buf[base + cube + off:base + 2 * cube + off].view(torch.float64)
            out.append(("one_buffer+%d" % off, tau, flux))
        return out

    res = {"npix": NPIX, "nchan": NCHAN, "reps": args.reps, "rounds": args.rounds,
           "offsets": list(OFFSETS), "builds": [b[0] for b in builds]}
    room = 2 * cube + OFFSETS[-1] + 8192
    buf = torch.empty(room, dtype=torch.uint8, device=eng.device)
    places = carve(buf)
    # bit equality of every build with the first, on the first placement
    _, tau, flux = places[0]
    launch(*builds[0], tau, flux)
    t0, f0 = tau.clone(), flux.clone()
    same = {}
    for b in builds[1:]:
        tau.zero_(), flux.zero_()
        launch(*b, tau, flux)
        eng.synchronize()
        same[b[0]] = {"tau": bool(torch.equal(tau.view(torch.int64), t0.view(torch.int64))),
                      "flux": bool(torch.equal(flux.view(torch.int64), f0.view(torch.int64))),
                      "ftot": bool(torch.equal(ftot[b[0]].view(torch.int64),
                                               ftot[builds[0][0]].view(torch.int64)))}
    del t0, f0
    res["bit_equal_to_" + builds[0][0]] = same
    print(json.dumps(same), flush=True)
    res["fresh"] = sweep(places)
    print(json.dumps({"fresh": res["fresh"]}), flush=True)
    # the fragmentation case: ~churn-gb allocated in 1 GiB chunks, two of every three freed AND
    # handed back to the driver (torch would otherwise keep them in its own cache, where a buffer
    # of more than 1 GiB cannot reuse them), the buffer allocated into what the driver has then,
    # the rest freed
    del places, tau, flux, buf
    torch.cuda.empty_cache()
    chunks = [torch.empty(1 << 30, dtype=torch.uint8, device=eng.device)
              for _ in range(args.churn_gb)]
    chunks = chunks[::3]
    torch.cuda.empty_cache()
    buf = torch.empty(room, dtype=torch.uint8, device=eng.device)
    del chunks
    torch.cuda.empty_cache()
    res["after_churn"] = sweep(carve(buf))
    print(json.dumps({"after_churn": res["after_churn"]}), flush=True)
    del buf
    # two allocations of their own (engine.ff_maps without `out`)
    tau, flux = eng._f64(1, NCHAN, NPIX), eng._f64(1, NCHAN, NPIX)
    res["separate"] = sweep([("separate(%+d)" % (flux.data_ptr() - tau.data_ptr() - cube), tau, flux)])
    res["separate_addresses"] = [hex(tau.data_ptr()), hex(flux.data_ptr())]
    print(json.dumps({"separate": res["separate"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
