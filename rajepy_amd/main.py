"""Command line of the radiative-transfer core, same flags as the reference's main.py:16-37:

    python -m rajepy_amd.main [-v] [-rt] [-so] [-r] [-c] model_params.py pipeline_params.py

`-so` observes every run that names a telescope on the device when `--antenna-configs DIR` (or the
environment variable RAJEPY_ANTENNA_CONFIGS) names a directory of simobserve antenna lists:
`--sefd JY` sets the thermal noise, `--seed N` its draw (`Pipeline.execute`).

`--formal` (not in the reference) writes the flux cubes of continuum runs by the formal solution
along the line of sight instead of the isothermal T_avg (1 - e^-tau); `--formal-rrl` does the same
for the flux cubes of radio-recombination-line runs (instead of B(T_avg) e^-tau_ff (1 - e^-tau_rrl)).

Several GPUs of one node: launch one process per GPU and the epochs of the run table are
shared out between them (each rank writes the products of its runs, rank 0 the state files):

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m rajepy_amd.main -rt model_params.py pipeline_params.py
"""
import argparse
import os
import runpy
import shutil
import time

from . import logger
from .classes import JetModel, Pipeline


def main(argv=None):
    parser = argparse.ArgumentParser(prog="rajepy_amd")
    parser.add_argument("model_param_file", help="Full path to model parameter file")
    parser.add_argument("pipeline_param_file", help="Full path to pipeline parameter file")
    parser.add_argument("-v", "--verbose", action="store_true",
                        help="Increase output verbosity")
    parser.add_argument("-rt", "--radiative-transfer", action="store_true",
                        help="Compute radiative transfer solutions")
    parser.add_argument("-so", "--simobserve", action="store_true",
                        help="Conduct synthetic observations on the device (needs "
                             "--antenna-configs or RAJEPY_ANTENNA_CONFIGS; skipped without)")
    parser.add_argument("--antenna-configs", default=None, metavar="DIR",
                        help="Directory of simobserve antenna lists (<tel>.<cfg>.cfg); default: "
                             "the environment variable RAJEPY_ANTENNA_CONFIGS")
    parser.add_argument("--sefd", type=float, default=None, metavar="JY",
                        help="System-equivalent flux density of one antenna [Jy] for the thermal "
                             "noise of the synthetic observations (default: noise-free)")
    parser.add_argument("--seed", type=int, default=0,
                        help="Seed of the thermal noise (run #i uses seed + i - 1)")
    parser.add_argument("-r", "--resume", action="store_true",
                        help="Resume previous pipeline run if present")
    parser.add_argument("-c", "--clobber", action="store_true",
                        help="Overwrite any data products/files present")
    parser.add_argument("--storage", choices=("f64", "f32"), default="f64",
                        help="HBM storage width of the 3-D fields")
    parser.add_argument("--formal", action="store_true",
                        help="Flux cubes by the formal solution along the line of sight "
                             "(observer at iy = 0) instead of the isothermal T_avg (1 - e^-tau); "
                             "continuum runs only")
    parser.add_argument("--formal-rrl", action="store_true",
                        help="Flux cubes of radio-recombination-line runs by the formal solution "
                             "along the line of sight (observer at iy = 0) instead of the "
                             "isothermal B(T_avg) e^-tau_ff (1 - e^-tau_rrl)")
    args = parser.parse_args(argv)
    jet_file = os.path.abspath(args.model_param_file)
    pline_file = os.path.abspath(args.pipeline_param_file)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RJP_DIST_BACKEND=gloo: rehearsal (e.g. several ranks sharing one GPU)
        backend = os.environ.get("RJP_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    dcy = os.path.expanduser(runpy.run_path(pline_file)["params"]['dcys']['model_dcy'])
    os.makedirs(dcy, exist_ok=True)
    log = logger.Log(os.sep.join([dcy, "ModelRun_" + time.strftime(
        "%Y-%m-%d-%H:%M:%S", time.localtime()) + ("_rank%d" % rank if world > 1 else "") +
        ".log"]), verbose=args.verbose)
    pline = Pipeline(JetModel(jet_file, log=log, storage=args.storage), pline_file, log=log)
    pline.log.add_entry("INFO", "Pipeline initiated using model parameters defined in {}, and "
                                "pipeline parameters defined in {}".format(jet_file, pline_file))
    pline.execute(resume=args.resume, clobber=args.clobber, simobserve=args.simobserve,
                  verbose=args.verbose, dryrun=not args.radiative_transfer, formal=args.formal,
                  formal_rrl=args.formal_rrl, antenna_configs=args.antenna_configs,
                  sefd_jy=args.sefd, seed=args.seed)
    for f in (jet_file, pline_file) if rank == 0 else ():
        dest = os.path.expanduser(os.sep.join([pline.params['dcys']['model_dcy'],
                                               os.path.basename(f)]))
        if f != dest:
            try:
                shutil.copyfile(f, dest)
            except shutil.SameFileError:
                print(f"{f} and {dest} are the same file")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return pline


if __name__ == '__main__':
    main()
