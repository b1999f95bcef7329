"""Host mirror of the crop helpers of ContextPose/mvn/utils/img.py: same names and
argument meaning, MI355X-native underneath (libcapf.so; no OpenCV, no CPU fallback for the warp)."""
import numpy as np

from capf import lib as _capf

IMAGENET_MEAN, IMAGENET_STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])    # img.py:8


def get_affine_transform(center, scale, rot, output_size, shift=np.array([0, 0], dtype=np.float32), inv=0):
    """img.py:16-48.  The reference only ever calls it with rot = 0, shift = 0, inv = 0 (crop_image, :63)."""
    if rot != 0 or inv != 0 or np.any(np.asarray(shift) != 0):
        raise ValueError("only rot = 0, shift = 0, inv = 0 (the reference's only call site, img.py:63) is supported")
    return _capf.affine_from_center_scale(center, scale, output_size)


def crop_image(image, center, scale, output_size):
    """img.py:51-69 for ONE frame: `image` is a uint8 CUDA tensor [H, W, 3]; returns a uint8 CUDA tensor
    [output_size[1], output_size[0], 3]."""
    return crop_image_batch([image], [center], [scale], output_size)[0]


def crop_image_batch(images, centers, scales, output_size):
    """What Human36M.__getitem__ (human36m.py:298-300) does per sample, for a whole batch in one launch:
    images: list of uint8 CUDA tensors [H_i, W_i, 3]; centers / scales: per-frame (x, y) pairs."""
    mats = np.stack([get_affine_transform(c, s, 0, output_size) for c, s in zip(centers, scales)])
    return _capf.warp_affine(list(images), mats, output_size)


def erase_image(image, center_list, size=70, use_mean=True):
    """img.py:179-198, the joint-centred cut-out behind the configuration's train.erase / val.erase: a square of side 2 * (size // 2) + 1
    around each centre of `center_list` that lies inside the image becomes the patch's own mean colour in the ORIGINAL image (use_mean) or 0;
    later centres paint over earlier ones.  `image`: uint8 [H, W, 3], a numpy array (uploaded, erased on the device, downloaded: a new
    array, as the reference returns) or a CUDA tensor (a new CUDA tensor).  Every centre goes through Python's own int() here, as in the
    reference (:188), before the device sees it, so a float64 centre such as 4.999999999999 truncates to 4 and a non-finite one raises; at most 32
    of them may lie inside the image (ValueError)."""
    import torch
    as_numpy = not torch.is_tensor(image)
    img = torch.as_tensor(np.ascontiguousarray(image)).cuda() if as_numpy else image
    H, W = img.shape[:2]
    # the reference's own test (:189) on the Python ints: what is left lies inside the image, where fp32 holds every column and row exactly
    pts = [(x, y) for x, y in ((int(x), int(y)) for x, y in center_list) if 0 <= x < W and 0 <= y < H]
    if len(pts) > _capf.ERASE_MAX_PATCHES or max(H, W) > 1 << 24:
        raise ValueError(f"at most {_capf.ERASE_MAX_PATCHES} centres inside an image of at most 2^24 columns and rows, got {len(pts)} in {W} x {H}")
    if not pts:
        out = img.clone()
    else:
        out = erase_image_batch(img.contiguous()[None], torch.tensor(pts, dtype=torch.float32, device=img.device).view(1, -1, 2), None, size, use_mean)[0]
    return out.cpu().numpy() if as_numpy else out


def erase_image_batch(images_u8, centers, mask=None, size=70, use_mean=True, out=None):
    """erase_image for a batch in one native call (capf_erase_patches): images_u8 uint8 CUDA [B, H, W, 3]; centers fp32 CUDA [B, P, 2] in crop
    pixels (the prefetcher's kcrop); mask uint8 / bool CUDA [B, P] or None: frame b is erased at centers[b, p] for the p with mask[b, p] != 0, in
    ascending p.  A centre counts iff -1 < x < W and -1 < y < H, the reference's truncation and range test on the fp32 values; a NaN or
    infinite centre is skipped where the reference raises.  out: None, images_u8 itself (in place) or a tensor of its own.  At most 32
    centres a frame (the project's joint cap): more raise CapfError."""
    return _capf.erase_patches(images_u8, centers, mask, size, use_mean, out)


def imread(path_or_bytes, device="cuda"):
    """cv2.imread(path, cv2.IMREAD_COLOR | cv2.IMREAD_IGNORE_ORIENTATION) of Human36M.__getitem__ (datasets/human36m.py:292-295) for a baseline
    JPEG: uint8 CUDA tensor [H, W, 3], BGR.  The host walks the Huffman stream, the GPU does the rest (capf_jpeg_decode); files this path does
    not take (progressive, CMYK, ...) raise CapfError -- there is no CPU fallback in this package."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    return _capf.jpeg_decode(bytes(data), device)


def _read_bytes(path_or_bytes):
    return bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()


def imread_batch(paths_or_bytes, device="cuda", subseq_bytes=0):
    """imread for a whole batch in ONE call, the Huffman decode on the GPU too (capf_jpeg_decode_batch): list of uint8 CUDA tensors
    [H_i, W_i, 3], BGR, the same bits as imread.  Synchronises once to read the per-file status and raises CapfError naming the files
    whose entropy data is corrupt (or, before any GPU work, the files outside the supported subset)."""
    items = list(paths_or_bytes)
    datas = [_read_bytes(p) for p in items]
    outs, status = _capf.jpeg_decode_batch(datas, device, subseq_bytes)
    bad = [(items[i] if not isinstance(items[i], (bytes, bytearray)) else f"#{i}", int(s)) for i, s in enumerate(status.cpu().tolist()) if s]
    if bad:
        raise _capf.CapfError(f"capf_jpeg_decode_batch: corrupt entropy data in {bad} (file, status bits)")
    return outs


def load_and_crop_batch(paths_or_bytes, centers, scales, output_size, device="cuda", decoder="host"):
    """The whole per-sample image path of Human36M.__getitem__ (human36m.py:292-300) for a batch: decode every frame on the GPU, then ONE
    warp launch for all crops.  Returns uint8 CUDA [B, output_size[1], output_size[0], 3], what the prefetcher (capf_preprocess) consumes.
    decoder="host": one imread per frame (host Huffman walk); "device": one imread_batch for all frames (same bits); "device_crop": one
    capf_jpeg_decode_crop_batch call for files -> crops, which transforms only the MCUs each crop reads and never builds a frame (same
    bits again; raises CapfError naming corrupt files, as imread_batch does)."""
    if decoder == "device_crop":
        items = list(paths_or_bytes)
        mats = np.stack([get_affine_transform(c, s, 0, output_size) for c, s in zip(centers, scales)])
        crops, status = _capf.jpeg_decode_crop_batch([_read_bytes(p) for p in items], mats, output_size, device)
        bad = [(items[i] if not isinstance(items[i], (bytes, bytearray)) else f"#{i}", int(s)) for i, s in enumerate(status.cpu().tolist()) if s]
        if bad:
            raise _capf.CapfError(f"capf_jpeg_decode_crop_batch: corrupt entropy data in {bad} (file, status bits)")
        return crops
    if decoder == "host":
        frames = [imread(p, device) for p in paths_or_bytes]
    elif decoder == "device":
        frames = imread_batch(paths_or_bytes, device)
    else:
        raise ValueError(f"decoder must be 'host', 'device' or 'device_crop', not {decoder!r}")
    return crop_image_batch(frames, centers, scales, output_size)
