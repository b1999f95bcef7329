"""GPU input preprocessing in front of the hot path: a mirror of `data_prefetcher`
(ContextPose/mvn/datasets/utils.py:15-89) — same constructor, same `.next()` contract, same side-stream
overlap — whose dozen elementwise torch ops are ONE native launch pair (capf_preprocess): uint8 BGR crop ->
normalised fp32 RGB NHWC, root-relative ground truth, train-time horizontal flip with left/right joint swap,
flip-test stacking.  The dataset / OpenCV side of the reference (human36m.py) is out of scope; any iterable
yielding (uint8 images [B,256,192,3], gt [B,1,17,3], k2d [B,17,2], kcrop [B,17,2]) CPU batches works.
`erase=` adds the joint-centred occlusion the configuration's train.erase / val.erase stand for (erase_image, mvn/utils/img.py:179-198; the
reference's dataset takes the flag and never calls the function) as one native call on the uint8 batch in front of that launch pair."""
import random

import torch

from capf import lib as _capf

joints_left = [4, 5, 6, 11, 12, 13]
joints_right = [1, 2, 3, 14, 15, 16]


class data_prefetcher():
    def __init__(self, loader, device, is_train, flip_test, backbone, fused_input=False, erase=None):
        """fused_input (an extension of the reference signature; False: the reference's contract, bit for bit): the image slot of
        next() holds the uint8 BGR batch itself, for CA_PF.forward_u8 -- no fp32 image is written.  The points still come mirrored /
        stacked / root-relative from the native launch (capf_preprocess_points), and `self.mirror` names the mode the batch returned
        by the LAST next() was prepared for: "all" when the train-time coin fell, "pair" for the flip test (the keypoints are then
        [2B,17,2], capf_preprocess mode 2's [2,B,17,2] flattened -- what forward_u8(mirror="pair") takes), else "none".
        erase (an extension too; None / False: today's launches and bits): True, or a dict with any of {size, use_mean, prob, joints,
        generator}.  On the side stream, before anything else, the raw uint8 batch is erased (capf_erase_patches) at the raw kcrop centres
        of the joints listed in `joints`, or, without that key, of each joint independently with probability `prob`, drawn with torch.rand on
        the device from `generator` (a CUDA torch.Generator; None: the device's default one).  size = 70 and use_mean = True are the reference
        function's defaults; prob = 0.5 is this project's choice, since the reference never wires the flag.  The mirrored train sample and both
        halves of the flip-test pair derive from the erased crop, as a dataset-side erase would have it; the labels are untouched.  With
        fused_input the image slot is the erased uint8 batch.  `self.erase_mask` holds the uint8 [B, 17] selection of the batch the LAST next()
        returned (None without erase)."""
        self.fused_input = fused_input
        self.erase = self._erase_options(erase)
        self.erase_mask = None
        self._next_erase_mask = None
        self.mirror = "none"
        self._next_mirror = "none"
        self.loader = iter(loader)
        self.stream = torch.cuda.Stream(device=device)
        self.device = device
        self.is_train = is_train
        self.flip_test = flip_test
        self.backbone = backbone
        self.preload()

    @staticmethod
    def _erase_options(erase):
        if erase is None or erase is False:
            return None
        opts = {"size": 70, "use_mean": True, "prob": 0.5, "joints": None, "generator": None}
        if erase is not True:
            unknown = set(erase) - set(opts)
            if unknown:
                raise ValueError(f"erase: unknown keys {sorted(unknown)} (known: {sorted(opts)})")
            opts.update(erase)
        if opts["joints"] is not None:
            opts["joints"] = sorted({int(j) for j in opts["joints"]})
            if opts["joints"] and not (0 <= opts["joints"][0] and opts["joints"][-1] < 17):
                raise ValueError(f"erase: joints must lie in [0, 17), got {opts['joints']}")
        if not 0.0 <= float(opts["prob"]) <= 1.0 or int(opts["size"]) < 0:
            raise ValueError(f"erase: prob must lie in [0, 1] and size must not be negative, got {opts['prob']}, {opts['size']}")
        return opts

    def _erase(self, images, kcrop):
        """the raw uint8 batch erased at the raw crop keypoints -> (a new uint8 batch, the uint8 [B, 17] selection)"""
        o = self.erase
        B, J = kcrop.shape[0], kcrop.shape[1]
        if o["joints"] is not None:
            mask = torch.zeros(B, J, dtype=torch.uint8, device=images.device)
            mask[:, o["joints"]] = 1
        else:
            mask = (torch.rand(B, J, device=images.device, generator=o["generator"]) < float(o["prob"])).to(torch.uint8)
        return _capf.erase_patches(images.contiguous(), kcrop.float().contiguous(), mask, int(o["size"]), bool(o["use_mean"])), mask

    def preload(self):
        try:
            batch = next(self.loader)
        except StopIteration:
            self.next_batch = None
            return
        with torch.cuda.stream(self.stream):
            images, gt, k2d, kcrop = [t.to(self.device, non_blocking=True) for t in batch]
            if self.erase is not None:
                images, self._next_erase_mask = self._erase(images, kcrop)
            if self.is_train and random.random() <= 0.5:              # utils.py:55
                mode = 1
            elif (not self.is_train) and self.flip_test:               # :67
                mode = 2
            else:
                mode = 0
            if self.fused_input:
                gt_o, k2d_o, kc_o = _capf.preprocess_points(gt.float(), k2d.float(), kcrop.float(), mode)
                if mode == 2:
                    k2d_o, kc_o = k2d_o.view(-1, 17, 2), kc_o.view(-1, 17, 2)
                self._next_mirror = ("none", "all", "pair")[mode]
                self.next_batch = [images.contiguous(), gt_o, k2d_o, kc_o]
                return
            img, gt_o, k2d_o, kc_o = _capf.preprocess(images, gt.float(), k2d.float(), kcrop.float(), self.backbone, mode)
            if mode == 2:     # the reference stacks on dim 1; [2,B,...] transposed is the same view without a copy
                img, k2d_o, kc_o = img.transpose(0, 1), k2d_o.transpose(0, 1), kc_o.transpose(0, 1)
            self.next_batch = [img, gt_o, k2d_o, kc_o]

    def next(self):
        torch.cuda.current_stream().wait_stream(self.stream)
        batch = self.next_batch
        self.mirror = self._next_mirror
        self.erase_mask = self._next_erase_mask
        if batch is not None:
            for t in batch:
                t.record_stream(torch.cuda.current_stream())
        self.preload()
        return batch
