#!/usr/bin/env python3
"""The reference's train.py:97-181 loop on the MI355X path, with synthetic VOC-shaped batches.

    python examples/train_like_train_py.py [--steps 20] [--amp] [--model MNFCOS] [--hip-stem] [--hip-bn-f16] [--hip-optim] [--ema 0.999] [--update-bn 8] [--assigner atss|simota] [--cls-loss qfl|vfl]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 examples/train_like_train_py.py   # DDP / RCCL

Same objects and call order as the reference: HalfInvertedStageFCOS([512, 1024, 2048], 20, 256), FCOSGenTargets,
FCOSLoss('giou'), SGD, DistributedDataParallel(find_unused_parameters=True), autocast + GradScaler, linear warm-up.
In model.train() the forward is an autograd graph of HIP kernels (train_ops.py); target assignment and the losses are HIP
kernels; under autocast the dense convolutions run on the f16 MFMA with fp32 accumulation (forward, data and weight gradients:
the reference's AMP arithmetic), normalisation and losses in fp32; under DDP the FPN's BatchNorms are SyncBatchNorm on the HIP statistics path.
--model MNFCOS (what the reference's config/main.yaml selects) builds MNFCOS([2048, 1024, 512], 20, 256) and opts in to its HIP training nodes
with model.enable_training() (which also freezes the Cin = 3 stem: the optimizer is built after it).  --hip-stem trains the 7x7 stem on its HIP node
(fd_stem7x7_bwd_weight_nhwc4) instead: MNFCOS keeps the stem trainable (enable_training(train_stem=True)), HISFCOS un-freezes conv1 and sets
enable_stem_training() -- without the option a trainable stem runs on stock ops.  --hip-bn-f16 (HISFCOS) builds the model with bn_freeze=False and calls
enable_stem_training().enable_trunk_batch_stats(f16_maps=True): the trunk's BatchNorms train on batch statistics on the HIP nodes and, with --amp, on f16
maps (fd_batchnorm_train_*_nhwc_h).  --hip-optim takes the optimizer from pytorch_object_detection_amd.optim:
step() on the HIP update kernels, GradScaler without a host read, and the warm-up / drop lines of train.py:160-173 evaluated on the device (optim.TrainPyLR)
instead of the host lines below.  --ema DECAY (with --hip-optim) keeps an exponential moving average of the weights in optim.AveragedModel, updated on the
device after every scaler.step(optimizer) -- a step GradScaler skips leaves it untouched -- and runs the averaged copy, avg.module, in eval mode at the end.
--update-bn N (with --ema) first runs optim.update_bn over N synthetic batches: the averaged copy holds averaged weights but only copied running
statistics, and its FPN BatchNorms run on batch statistics; update_bn recomputes exactly those on the HIP kernels (every rank passes its own batches under
DDP: the statistics are global) and leaves the frozen backbone's alone.  --assigner atss replaces the one line train.py:98 by ATSSGenTargets(strides):
Adaptive Training Sample Selection on the device (fd_atss_gen_targets) instead of the scale ranges and the centre radius; --assigner simota by SimOTAGenTargets(strides): SimOTA on the device (fd_simota_gen_targets),
which ranks the locations inside a box by the score and the box the model currently predicts there; nothing else changes.
--cls-loss qfl | vfl replaces the hard-label focal term by Quality Focal Loss or Varifocal Loss (FCOSLoss('giou', cls_mode=...), fd_quality_loss_fwd / _bwd):
the losses GFL and VarifocalNet train with, e.g. `--assigner simota --cls-loss qfl`.
"""
import argparse
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_object_detection_amd import optim  # noqa: E402
from pytorch_object_detection_amd.model.loss import FCOSLoss  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import ATSSGenTargets, FCOSGenTargets, SimOTAGenTargets  # noqa: E402
from pytorch_object_detection_amd.model.od import MNFCOS, HalfInvertedStageFCOS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--amp", action="store_true")
    ap.add_argument("--model", choices=["HISFCOS", "MNFCOS"], default="HISFCOS")
    ap.add_argument("--hip-stem", action="store_true", help="train the 7x7 stem (conv1) on its HIP forward / weight-gradient node")
    ap.add_argument("--hip-bn-f16", action="store_true",
                    help="HISFCOS with bn_freeze=False: the trunk's BatchNorms on batch statistics on the HIP nodes, on f16 maps under --amp")
    ap.add_argument("--hip-optim", action="store_true", help="optim.SGD with the learning-rate rule on the device instead of torch.optim.SGD and the host lines")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY", help="average the weights on the device (optim.AveragedModel); needs --hip-optim")
    ap.add_argument("--update-bn", type=int, default=0, metavar="N",
                    help="recompute the averaged copy's batch-statistics BatchNorms over N batches before its eval forward (optim.update_bn); needs --ema")
    ap.add_argument("--assigner", choices=["fcos", "atss", "simota"], default="fcos",
                    help="target assignment: FCOSGenTargets (train.py:98), ATSSGenTargets or SimOTAGenTargets")
    ap.add_argument("--cls-loss", choices=["focal", "qfl", "vfl"], default="focal",
                    help="classification term: the reference's focal loss, Quality Focal Loss or Varifocal Loss (e.g. --assigner simota --cls-loss qfl)")
    args = ap.parse_args()
    if args.ema is not None and not args.hip_optim:
        ap.error("--ema gates on the HIP optimizer's skip flag: pass --hip-optim as well")
    if args.hip_bn_f16 and args.model != "HISFCOS":
        ap.error("--hip-bn-f16 is for --model HISFCOS (the ResNet-50 trunk's switch)")
    if args.update_bn < 0 or (args.update_bn and args.ema is None):
        ap.error("--update-bn N (N >= 1) recomputes the statistics of the averaged model: pass --ema as well")
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("WORLD_SIZE", 1), ("LOCAL_RANK", 0)))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    torch.manual_seed(0)
    if args.model == "MNFCOS":
        model = MNFCOS([2048, 1024, 512], 20, 256).enable_training(train_stem=args.hip_stem).to(dev)   # config/main.yaml:2, mnfcos.yaml
    elif args.hip_bn_f16:
        model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats(f16_maps=True).to(dev)
    else:
        model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(dev)                           # train.py:97
        if args.hip_stem:
            model.backbone.conv1.weight.requires_grad_(True)      # (the constructor's freeze_stages(1) froze it; bn1 stays frozen and folds into the launch)
            model.enable_stem_training()
    gen_target = FCOSGenTargets(strides=[8, 16, 32, 64, 128],
                                limit_range=[[-1, 64], [64, 128], [128, 256], [256, 512], [512, 999999]])   # train.py:98
    if args.assigner == "atss":
        gen_target = ATSSGenTargets(strides=[8, 16, 32, 64, 128])
    elif args.assigner == "simota":
        gen_target = SimOTAGenTargets(strides=[8, 16, 32, 64, 128])
    if world > 1:
        model = torch.nn.parallel.DistributedDataParallel(model, find_unused_parameters=True)       # train.py:101
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)                                 # train.py:103
    LR_INIT, WARMUP_STEPS = 1e-3, 501
    trainable = [p for p in model.parameters() if p.requires_grad]
    if args.hip_optim:
        optimizer = optim.SGD(trainable, lr=LR_INIT, momentum=0.9, weight_decay=1e-4, lr_schedule=optim.TrainPyLR(LR_INIT, WARMUP_STEPS))
    else:
        optimizer = torch.optim.SGD(trainable, lr=LR_INIT, momentum=0.9, weight_decay=1e-4)
    # train.py:125 (commented out there): the averaged copy; pairs by position, so the DDP wrapper's parameters pair with the bare copy's
    avg = optim.AveragedModel(model.module if world > 1 else model, decay=args.ema, optimizer=optimizer) if args.ema is not None else None
    scaler = torch.amp.GradScaler("cuda", enabled=args.amp)                                         # train.py:133
    criterion = FCOSLoss("giou", cls_mode=args.cls_loss)       # "qfl" / "vfl": the class target of a positive is the IoU of its current box prediction

    g = torch.Generator(device=dev).manual_seed(100 + rank)      # synthetic batches are drawn on the device (no dataloader here)
    model.train()
    t0 = None
    for step in range(1, args.steps + 1):
        imgs = torch.randn(args.batch, 3, 512, 512, generator=g, device=dev)                            # collate_fn output shape
        c = torch.rand(args.batch, 8, 2, generator=g, device=dev) * 400 + 50
        s = torch.rand(args.batch, 8, 2, generator=g, device=dev) * 150 + 20
        targets = torch.cat([c - s / 2, c + s / 2], -1).clamp(0, 511)
        classes = torch.randint(1, 21, (args.batch, 8), generator=g, device=dev)
        if step < WARMUP_STEPS and not args.hip_optim:                                              # train.py:161-164
            for group in optimizer.param_groups:
                group["lr"] = float(step / WARMUP_STEPS * LR_INIT)
        optimizer.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16, enabled=args.amp):                         # train.py:175-179
            outputs = model(imgs)
            target = gen_target([outputs, targets, classes])
            losses = criterion([outputs, target])
            loss = losses[-1]
        scaler.scale(loss.mean()).backward()
        scaler.step(optimizer)
        scaler.update()
        if avg is not None:
            avg.update_parameters(model)                                                            # train.py:203; after the step: the gate reads its skip flag
        if step == 3:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if rank == 0 and (step % 5 == 0 or step == 1):
            print(f"step {step:4d}  cls {float(losses[0]):.4f}  cnt {float(losses[1]):.4f}  reg {float(losses[2]):.4f}  "
                  f"total {float(losses[3]):.4f}  mem {torch.cuda.memory_reserved() / 1e9:.2f} GB")
    torch.cuda.synchronize()
    if rank == 0 and t0 is not None and args.steps > 3:
        dt = (time.perf_counter() - t0) / (args.steps - 3)
        print(f"{dt * 1e3:.1f} ms/step, {args.batch * world / dt:.1f} img/s over {world} GPU(s)")
    if avg is not None and args.update_bn:                      # on every rank: SyncBatchNorm's statistics are collective
        optim.update_bn((torch.randn(args.batch, 3, 512, 512, generator=g, device=dev) for _ in range(args.update_bn)), avg)
        if rank == 0:
            print(f"update_bn: the averaged model's batch-statistics BatchNorms recomputed over {args.update_bn} batches")
    if avg is not None and rank == 0:
        with torch.no_grad():
            cls_logits = avg.module.eval()(imgs)[0]                                                 # the averaged weights, on their own plans
        print(f"averaged model after {int(avg.n_averaged)} updates: largest class logit {max(float(t.max()) for t in cls_logits):.4f}")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
