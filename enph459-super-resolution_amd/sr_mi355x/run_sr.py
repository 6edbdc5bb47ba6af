"""`python -m sr_mi355x.run_sr` -- the reference's `python run_sr.py` on the MI355X.

Same four flags as the reference's drivers (mono_cal_target/run_sr.py:320-331: --psf {gaussian,measured},
--psf-dir, --data-dir, --output-dir) plus --kind, because the reference has one script per experiment layout
while this is one entry point, and --precision.

Several GPUs: launch it under torchrun, one process per GPU --
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m sr_mi355x.run_sr --kind ... --data-dir ...
Session i goes to rank i mod G (the reference's outer loop order, mono_cal_target/run_sr.py:358-360); the ranks share nothing
but the output directory, so there is no collective on the data path, only a barrier before rank 0 reports the total time.
RANK / LOCAL_RANK / WORLD_SIZE are read, and the device chosen, BEFORE the first GPU call.
--row-bands (cal_target kinds) is the other mode: every rank walks all sessions and each image's IBP loop is split into row bands
whose halo rows travel point to point between neighbouring ranks (sr_mi355x/rowband.py; RCCL send/recv on the GPUs).
"""
import argparse
import os
import time

from . import api, session


def main(argv=None):
    ap = argparse.ArgumentParser(description="Multi-frame super-resolution (Native-2x, SAA, SAA+IBP) on an MI355X")
    ap.add_argument("--kind", required=True, choices=sorted(session.IBP_ITERATIONS),
                    help="experiment layout = which of the reference's run_sr.py drivers to mirror")
    ap.add_argument("--psf", choices=["gaussian", "measured"], default="gaussian")
    ap.add_argument("--psf-dir", default=None, help="pinhole calibration images (sweep*/pos4_(0,0).png)")
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--precision", choices=["f32", "f64"], default="f32")
    ap.add_argument("--metrics", action="store_true",
                    help="mono_cal_target only: also write metrics.json (slanted-edge MTF50/MTF10, bar contrast: the "
                         "summary of the reference's analysis.ipynb) next to the PNGs")
    ap.add_argument("--metrics-on-device", action="store_true",
                    help="with --metrics: the whole report is queued on the device (srx_edge_sfr: percentile, line fits, ESF, MTF50 / MTF10 "
                         "of the three ROIs in one call) and metrics.json is written by a worker thread; the main thread waits for nothing")
    ap.add_argument("--row-bands", action="store_true",
                    help="several GPUs on ONE image: split every image's IBP loop into row bands (cal_target kinds; under torchrun)")
    ap.add_argument("--register", action="store_true",
                    help="estimate the frames' shifts on the device (table as the start) and reconstruct with them; "
                         "writes registration.json next to the PNGs (barcode kinds: the reps of a session still go through the "
                         "library as one batch, every rep under its own table)")
    ap.add_argument("--psf-on-device", action="store_true",
                    help="with --psf measured: estimate the PSF from the pinhole frames on the device (uint8 frames uploaded as they are)")
    ap.add_argument("--u8-frames", action="store_true",
                    help="keep the 8-bit frames as bytes on the device (every kind): shift_and_add and ibp read them through srx_saa_u8lr / "
                         "srx_ibp_u8lr, with --register registration through srx_register_u8, and the frame mean and rgb_cal_target's rep "
                         "mean of the red planes through srx_mean_u8; the files written are the same")
    ap.add_argument("--png-on-device", action="store_true",
                    help="build the output PNGs on the device (srx_png_file: quantise, Up filter, run lengths and Huffman coding per "
                         "32 KB chunk, the container and its CRC-32); the host only writes the bytes.  Same pixels in every file, other bytes")
    ap.add_argument("--patchwise", choices=["global", "local"], default=None,
                    help="cal_target kinds: reconstruct in overlapping 256 x 256 HR patches that are blended back (sr_mi355x/patchwise.py).  "
                         "local: every patch under the shifts registered on it, the shift field written as shift_field.json next to the "
                         "PNGs; global: every patch under the session's one table (the baseline of local)")
    ap.add_argument("--colour", action="store_true",
                    help="the two rgb_* kinds: reconstruct all four Bayer planes (one batch under the one table; with --register the shifts "
                         "measured on the red planes) and write native_2x_rgb.png, SAA_rgb.png, SAA_IBP_rgb.png and "
                         "convergence_planes.json beside the files of the plain run, which do not change.  Goes with --u8-frames, "
                         "--register and --png-on-device; not with --patchwise or --row-bands")
    args = ap.parse_args(argv)
    if args.metrics_on_device and not args.metrics:
        ap.error("--metrics-on-device needs --metrics")
    if args.colour and args.kind not in ("rgb_cal_target", "rgb_barcodes"):
        ap.error("--colour is for the two rgb_* kinds (raw RGGB frames)")
    if args.colour and (args.patchwise or args.row_bands):
        ap.error("--colour goes with neither --patchwise nor --row-bands")
    if args.patchwise and args.row_bands:
        ap.error("--patchwise and --row-bands exclude each other")
    if args.patchwise and args.kind not in ("mono_cal_target", "rgb_cal_target"):
        ap.error("--patchwise is for the cal_target kinds (one large image per session)")
    rank, world, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:  # one process per GPU: pick the device before anything touches it
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0 if os.environ.get("SRX_ONE_GPU") else local_rank)  # SRX_ONE_GPU: rehearsal of the N > 1 path on a one-GPU box
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # item sharding: a barrier and nothing else (gloo).  Row bands: halo rows as CUDA tensors over RCCL, host objects over gloo
        dist.init_process_group("cpu:gloo,cuda:nccl" if args.row_bands and not os.environ.get("SRX_ONE_GPU") else "gloo")
    api.set_precision(args.precision)
    if args.psf == "measured":
        if not args.psf_dir:
            ap.error("--psf measured needs --psf-dir")
        psf = (session.load_measured_psf_device if args.psf_on_device else session.load_measured_psf)(args.psf_dir)
        print(f"  PSF: measured{' on the device' if args.psf_on_device else ''}, kernel shape {psf.shape}")
    else:
        if args.psf_on_device:
            ap.error("--psf-on-device needs --psf measured")
        psf = api.make_gaussian_psf(session.PSF_SIZE, session.PSF_SIGMA)
        print(f"  PSF: Gaussian {session.PSF_SIZE}x{session.PSF_SIZE}, sigma={session.PSF_SIGMA}")
    sessions = session.discover_sessions(args.data_dir, args.kind)
    print(f"Found {len(sessions)} session(s):\n" + "\n".join(f"  {os.path.basename(s)}" for s in sessions))
    t0 = time.time()
    # --metrics: from the device tensors the PNGs were quantised from (session.write_metrics_device), not from the files;
    # --metrics-on-device: the same report queued whole (session.queue_metrics_device)
    metrics_cb = None
    if args.metrics and args.kind == "mono_cal_target":
        metrics_cb = session.queue_metrics_device if args.metrics_on_device else session.write_metrics_device
    session.process_sessions(sessions, psf, args.output_dir, args.kind, rank=rank, world=world, on_images=metrics_cb,
                             row_bands=args.row_bands and world > 1, register=args.register,
                             keep_u8=args.u8_frames, device_png=args.png_on_device, patchwise=args.patchwise, colour=args.colour)
    if dist is not None:
        dist.barrier()
    if rank == 0:
        print(f"\nAll sessions done in {(time.time() - t0) / 60:.1f} min" + (f" on {world} GPUs" if world > 1 else ""))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
