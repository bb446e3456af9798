#!/usr/bin/env python3
"""Everything that describes the C ABI, generated from the MOPA_API definitions in csrc/*.hip, which are parsed once (`parse`):

  include/mopa_hip.h            the prototypes (the section comments -- which reference interface each group replaces -- are
                                maintained here)
  mopa_amd/csrc/exec_table.inc  the dispatch table of the command-list executor (exec2d.hip)
  mopa_amd/_abi.py              the ctypes signatures of mopa_amd/_lib.py and the host-pointer parameters of every entry point

`generate()` returns the three texts, `main()` writes them; tests/test_cabi.py asserts that the committed files are what it returns."""
import collections
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))

SECTIONS = [
    ("hash3d.hip", """Voxel hash, active sets and rule tables (integer; bit-exact with oracle/scn3d.py::Geometry).
 * Replaces sparseconvnet's host-side Metadata (hash map + rulebooks) reached through
 *   mopa/models/scn_unet.py:26  scn.InputLayer(3, full_scale, mode=4)        -> mopa_voxel_hash_build, mopa_points_csr
 *   mopa/models/scn_unet.py:27  scn.SubmanifoldConvolution(3, cin, m, 3)      -> mopa_rulebook_subm
 *   mopa/models/scn_unet.py:28  scn.UNet(...) Convolution / Deconvolution 2,2  -> mopa_coarsen_build, mopa_rulebook_updown
 * Input contract: coords (N,4) int64 [x,y,z,batch] (mopa/data/collate.py:183-185), 0 <= x,y,z < 4096."""),
    ("spconv.hip", """Sparse convolution on rule tables nbr[K][num_out] (int32, -1 = no rule): out[i] = sum_o in[nbr[o][i]] @ W[o].
 * Replaces the gather-GEMM-scatter kernels of sparseconvnet behind
 *   mopa/models/scn_unet.py:27-28 (SubmanifoldConvolution K=27; scn.UNet Convolution / Deconvolution K=8)
 * forward / backward-data: mopa_spconv_fwd (backward-data = same call on the reversed table with transposed weights);
 * backward-weight: mopa_spconv_bwd_weight."""),
    ("sprun.hip", """The same convolutions, offset-major: run-major rulebook (the rules of one filter offset are one contiguous run of slots),
 * per-offset gather-GEMM with the weight slice resident in LDS, products into a partial slab, one ordered per-row sum -- for the
 * launches the matrix pipe bounds (same reference call sites as spconv.hip; SURVEY A.8 "gather-GEMM-scatter")."""),
    ("exec2d.hip", """Command-list executor: a recorded sequence of this library's own entry points (plus event record / wait between two
 * streams) replayed in ONE call -- the 2D branch's forward / backward pass (mopa/models/resnet34_unet.py:131-191 behind
 * mopa/models/xmuda_arch.py:49-79) without one interpreter round trip per launch; recorder: mopa_amd/dense2d.py::Graph2D."""),
    ("scn_exec.hip", """Native executor of the 3D branch: the whole UNetSCN forward / backward (scn.Sequential of mopa/models/scn_unet.py:25-30
 * with scn.UNet unrolled + the linear heads of mopa/models/xmuda_arch.py:114-126) as ONE call each over host-side tables
 * (layer program, parameter pointers, rule tables, buffer addresses); table layouts: scn_exec.hip / mopa_amd/sparse3d.py."""),
    ("rows.hip", """Row-wise ops over active rows [rows][C] (row stride ld): BatchNorm(+residual)(+Leaky)ReLU, InputLayer, OutputLayer+heads.
 * Replaces  scn.BatchNormReLU / BatchNormLeakyReLU (mopa/models/scn_unet.py:28-29; eps 1e-4),
 *           torch.nn.BatchNorm2d + ReLU (+ residual add of torchvision BasicBlock) of mopa/models/resnet34_unet.py:95,115-129,
 *           scn.InputLayer mode 4 / scn.OutputLayer (mopa/models/scn_unet.py:26,30),
 *           nn.Linear heads on per-point features (mopa/models/xmuda_arch.py:73-77,116,124) and the integer point
 *           gather x[i][idx[:,0], idx[:,1]] (mopa/models/xmuda_arch.py:62-65) -> mopa_output_layer_heads_{fwd,bwd}."""),
    ("conv2d.hip", """Dense 2D convolution (NHWC fp32 implicit GEMM; f32-operand MFMA by default, the fp32 vector pipe with MOPA_CONV2D_MFMA=0): Conv2d fwd / backward-data / backward-weight and
 * ConvTranspose2d(k2,s2) through one index map (25 x int32 'geom', see conv2d.hip::ConvGeom).
 * Replaces the cuDNN calls behind mopa/models/resnet34_unet.py:93 (conv1 7x7), :97-101 (layer1-4), :104-110,:115-129 (decoder)."""),
    ("wino2d.hip", """Winograd F(2x2,3x3) transforms for the stride-1 3x3 convolutions with >= 128 channels (same reference call sites as
 * conv2d.hip); the 16 point-wise GEMMs run through mopa_conv2d_igemm_batched."""),
    ("wino4c9.hip", """The same one-kernel F(4x4) convolution as mopa_wino4_conv (wino2d.hip), nine transform points per wave on v_mfma_f32_32x32x2_f32:
 * half the weight bytes per tile and a quarter of the weight loads per matrix instruction (same reference call sites)."""),
    ("wino4wg.hip", """Weight gradient of the stride-1 3x3 convolutions through Winograd F(4x4,3x3) in ONE kernel (x and dY in, dW out: neither
 * transformed operand reaches HBM) -- torch autograd's conv2d weight gradient of layer1's BasicBlocks and the decoder's 3x3
 * convolutions (mopa/models/resnet34_unet.py:97,104-110,176-182); mopa_wino4_bwd_weight (conv2d.hip) is the two-operand form."""),
    ("ops2d.hip", """MaxPool 3x3/s2/p1 (resnet34_unet.py:148), Dropout p=0.4 (:154,:159), full-image linear head
 * (mopa/models/xmuda_arch.py:58-60), column sums for conv-bias gradients (decoder convs have bias=True, :104-110)."""),
    ("losses.hip", """Losses: cross-modal KL (mopa/train/train_xmuda_mopa.py:389-398,440-445), weighted CE with ignore_index -100
 * (:354-363,456-465,563-567), softmax over classes (:473) and mask_cons_loss (mopa/common/utils/loss.py:241-283).
 * Loss scalars, normalisers and upstream gradients are device pointers (no host sync)."""),
    ("coral.hip", """logCORAL loss on the device: logcoral_loss of mopa/models/losses.py:47-93 (TRAIN.XMUDA.lambda_logcoral), float64 arithmetic
 * on float32 features of width 1 <= F <= 64.  Forward: column means and centred Gram matrices of both inputs (a fixed number of
 * blocks walk the rows; float64 partial slabs summed in index order), cov = Gram / (batch_size - 1) for BOTH inputs with
 * batch_size = x_src.shape[0] before flattening, the reference's guard (an entry > 1e30 or NaN in either covariance turns both into
 * the identity), a parallel cyclic two-sided Jacobi eigendecomposition in LDS (one workgroup per matrix, bounded sweeps),
 * L = V diag(log|lambda|) V^T, loss = mean((L_src - L_trg)^2), and per input S = factor (dC + dC^T) from the divided-difference form of
 * the matrix logarithm's derivative, kept with the means in `state`.  Backward: dX = g (x - mean) S per row, exact zeros under the
 * guard.  No floating-point atomics: the same bits on every run.  `status` (int32 on the device, never read back by the call): bit 0 the
 * guard fired, bit 1 Jacobi hit its sweep bound, bit 2 an eigenvalue was <= 0.  The arithmetic is stated in DESIGN.md section 4;
 * yardstick tests/_coral_reference.py, held against the reference's float64 autograd."""),
    ("lovasz.hip", """Lovasz-softmax loss on the device: lovasz_softmax / Lovasz_softmax of mopa/common/utils/loss.py:107-199, for float32
 * probabilities (P, C) with 2 <= C <= 64, or from logits (the probabilities are formed on the fly with mopa_softmax_fwd's bits and
 * never stored).  Per (row segment, class): key e = |fg - p| (one float32 operation), a stable LSD radix sort of (key bits, row)
 * pairs -- descending e, equal keys in ascending row order, ignored rows last -- with per-block digit histograms in LDS and scatter
 * offsets from a scan of the block x digit table, integer running counts of the foreground along the order, float64 Jaccard weights
 * w_k = J_k - J_{k-1}, L_c = sum e_k w_k in float64 in a fixed order; the loss is the mean over the selected classes and then over
 * the segments ('present' / 'all' / a list; up to 32 segments for per_image=True).  sign(p - fg) w goes into a coefficient plane,
 * all the backward reads.  Class and segment are grid dimensions: the same launches for every P, C and label content; a class that
 * is not selected costs no sort work; no host read, no floating-point atomics: the same bits on every run.  `status` (int32 on the
 * device): bit 0 a label outside [0, C) that is not the ignore value (foreground for no class).  The arithmetic is stated in
 * DESIGN.md section 4; yardstick tests/_lovasz_reference.py, held against the reference's own float32 result."""),
    ("supcon.hip", """Supervised contrastive loss on the device: SupConLoss of mopa/models/losses.py:123-184 (TRAIN.PC_MM.lambda_ctr_src /
 * lambda_ctr_trg) and l2_norm of mopa/common/utils/loss.py:230-238, for float32 features of width 1 <= F <= 128 and int64 labels
 * compared for equality only.  With S = A Q^T / T, per anchor m = max_j S, D = sum over negatives of (exp(S - m) + float32(1e-5)),
 * loss = -mean_i ((1 / n_i) sum over positives of (S - m) - log D); no self-pair exclusion.  Nothing of size Na x Nq exists: the
 * forward is one launch over (anchor tiles of 64) x (pool chunks) whose S tiles stay in the accumulators of v_mfma_f32_32x32x2_f32
 * (features staged through LDS, odd widths zero padded there), with a running maximum and rescaled sums per row, and one finalize
 * launch that merges the chunks in order and sums the rows in float64; the backward is one launch per side (anchors: side 0, pool:
 * side 1) that recomputes the S tiles and multiplies W = [P] / n - [N] exp(S - m) / D on the same instruction, plus one ordered sum
 * when the walk was split for occupancy.  The number of chunks depends on (Na, Nq) alone (mopa_supcon_pool_chunks); no
 * floating-point atomics: the same bits on every run.  An anchor without a positive or without a negative is invalid: the loss is NaN
 * and every gradient element NaN (skip_invalid = 0), or the row is left out of the mean (skip_invalid = 1; none valid: 0).
 * `status` (int32 on the device, never read back by the call): bit 0 an anchor has no positive, bit 1 an anchor has no negative,
 * bit 2 a non-finite S was met.  The arithmetic is stated in DESIGN.md section 4; yardstick tests/_supcon_reference.py, held against
 * the reference's float64 autograd."""),
    ("pseudo.hip", """Pseudo-label update of the MoPA phase on the device (SURVEY 8f-3): EMA teacher (torch_ema update rule,
 * mopa/train/train_xmuda_mopa.py:221-226,587-591), entropy-weighted 2D/3D fusion (:282-291 with mopa/models/losses.py:10-19)
 * and the per-class median refinement (mopa/data/utils/refine_pseudo_labels.py:5-22), without host round trips."""),
    ("vgi.hip", """Valid Ground-based Insertion on the device (SURVEY 8f-4): overlap test of the object's box against the scan's
 * occupancy (mopa/data/mixmatch_ss.py:215-331 check_overlap), centre filters (:139-160), ground-cell lookup and road height
 * (:355-455 obj_on_road), range-image occlusion culling (mopa/data/utils/augmentation_3d.py:81-111,161-290) and the float64
 * voxeliser of post_process (mixmatch_ss.py:458-559)."""),
    ("evaluate.hip", """Validation metrics on the device: predictions, confusion matrices, logged entropy means and CE losses, pseudo-label dump
 * (mopa/data/utils/validate.py:112-170,184-185) and Evaluator.update (mopa/data/utils/evaluate.py:12-26: sklearn confusion_matrix
 * with labels=) without host round trips.  Confusion matrices are int64 (n_labels, n_labels), rows = ground truth, added to."""),
    ("imageprep.hip", """The 2D half of the input pipeline on the device: Pillow's 8-bit BILINEAR resize, the three ImageEnhance blends behind
 * torchvision's ColorJitter, flip + /255. + normalisation into the CHW batch tensor, scipy's order-0 zoom + refine_sam_mask, and
 * the image-index transforms of Dataset.__getitem__ (mopa/data/nuscenes/nuscenes_dataloader.py:347-408,
 * mopa/data/semantic_kitti/semantic_kitti_dataloader.py:563-630, mopa/data/utils/refine_pseudo_labels.py:72-102); bit-exact.
 * Per-image pointers and draws are small host arrays (at most 32 images per call); one launch per stage for the whole batch."""),
    ("denselabels.hip", """Dense 2D pseudo labels from SAM masks on the device, all samples of a call per launch: refine_sam_2Dlabels
 * (mopa/data/utils/refine_pseudo_labels.py:25-69) behind the row expansion of SemanticKITTISCN.preprocess
 * (mopa/data/semantic_kitti/semantic_kitti_dataloader.py:443-451) and the crop + flip of __getitem__ (:587-590,:611-613): maximum
 * and first arg-max of the never-built (N, C) rows, the per-class median refinement (mopa_refine_pseudo_labels_segmented, one segment
 * per image), the scatter in which the last point of a pixel wins, per mask id the pixel count and the class sums of the winning
 * rows (int64 fixed point, 2^-40 units, integer atomics: the same bits on every run), the fill of every id below the area
 * threshold with its first arg-max, and the crop window and flip in the store.  Equal to the reference wherever the float64 sums
 * decide an id (DESIGN.md section 4); points outside the image, with a raw label >= C or a probability outside [0, 1] are skipped
 * and counted per image on the device.  Per-image pointers and draws are small host arrays (at most 32 images per call); the same
 * number of launches for every batch size; no read-back."""),
    ("scanprep.hip", """The 3D half of the input pipeline on the device, all scans of an iteration per launch: rotation, voxel coordinates
 * and in-field filter of augment_and_scale_3d + Dataset.__getitem__ (mopa/data/utils/augmentation_3d.py:48-59,
 * mopa/data/nuscenes/nuscenes_dataloader.py:339-340,410-465, mopa/data/semantic_kitti/semantic_kitti_dataloader.py:583-585,632-676),
 * one ordered compaction of every per-point array into the layout of collate_scn_base (mopa/data/collate.py:182-264) and
 * refine_pseudo_labels (mopa/data/utils/refine_pseudo_labels.py:5-22) for many (array, scan) segments at once; same bits as
 * mopa_rotate_points_f32 + mopa_voxelize per scan.  Per-scan pointers, sizes and draws are small host arrays (at most 32 scans,
 * 64 segments per call)."""),
    ("kittiprep.hip", """SemanticKITTI's on-the-fly projection on the device, all scans of an iteration per launch: the z > -3 filter, the low 16
 * label bits, the ground mask from PatchWork++'s index list, the front-half filter, proj_matrix times the homogeneous points (per
 * row the fused chain fma(m3, 1, fma(m2, z, fma(m1, y, m0 * x)))), the perspective divide, np.around(., 2), the strict frustum
 * test and one ordered compaction of every per-point array -- data_extraction and preprocess of
 * mopa/data/semantic_kitti/semantic_kitti_dataloader.py:349-371,422-507 with select_points_in_frustum (:236-252); the pseudo-label
 * form (:430-469) takes the loaded keep mask instead of projecting.  Per-scan pointers and matrices are small host arrays (at most
 * 32 scans per call); the caller reads back the 2 B counts once, between mopa_kittiprep_count and mopa_kittiprep_scatter."""),
    ("nuscprep.hip", """nuScenes' offline preprocessing of a sweep on the device, all sweeps of a call per launch: the float64 lidar -> ego ->
 * global -> ego(cam) -> camera chain, the intrinsics, the perspective divide, the float32 cast and the strict frustum test of
 * map_pointcloud_to_image (mopa/data/nuscenes/projection.py:9-90), the detection labels painted from the 3D boxes (the last
 * labelled box that holds a point wins; mopa/data/nuscenes/preprocess.py:116-126 with the devkit's points_in_box), one ordered
 * compaction (preprocess.py:111-114) and the ground mask of mopa/data/nuscenes/nuscenes_dataloader.py:305-316 (index lists go
 * through mopa_kittiprep_ground).  Every matrix product is per element the fused chain fma(a[K-1], b[K-1], ... a0 * b0); rotation
 * matrices, viewpad and the box frames are computed on the device (mopa_nuscprep_setup) from the quaternions, in a small table.
 * Per-scan pointers are small host arrays (at most 32 scans per call, any number of boxes); the caller reads back the B counts
 * once, between mopa_nuscprep_count and mopa_nuscprep_scatter."""),
    ("a2d2prep.hip", """A2D2's offline preprocessing of a frame on the device, all frames of a call per launch: undistort_image and
 * DummyDataset.__getitem__ of mopa/data/a2d2/preprocess.py:26-44,96-141 -- cv2.undistort of the Telecam image and of the
 * colour-coded label image as an inverse map built once per camera (float64, every operation rounded once; stored in OpenCV's
 * CV_16SC2 + CV_16UC1 fixed-point layout, INTER_BITS = 5) and a bilinear remap with a constant 0 border (integer; the closed form
 * of cv2.remap's 15-bit weight table), the label image read at every lidar point's [int32(row), int32(col)] (remapped on the
 * spot, the same bytes as the full plane), the RGB code -> class index lookup of class_list.json (the last equal row wins, else
 * K) and the float32 casts of points, reflectance / 255 and points_img.  The chain is stated in DESIGN.md section 4; yardstick
 * tests/_a2d2_reference.py; OpenCV itself was not at hand.  Per-plane and per-frame pointers are small host arrays (at most 64
 * planes, 32 frames per call); points outside the label image get K and are counted per frame on the device; no read-back."""),
    ("jpegdec.hip", """JPEG decoding split at the quantised coefficients -- np.asarray(Image.open(img_path)) in front of the 2D pipeline
 * (mopa/data/nuscenes/nuscenes_dataloader.py:347-349), Pillow's bits.  Host half (csrc/jpeg_entropy.h, plain C++, no GPU needed):
 * marker parser and Huffman decoding of baseline sequential streams (8-bit; 1 component, or 3 with chroma 1 x 1 and luma 1 x 1,
 * 2 x 1 or 2 x 2; one interleaved scan; restart intervals; sides up to 8192) into int16 [blocks_y][blocks_x][64] planes in natural
 * order behind the quantisation tables, and a JpegHeader (geometry, sampling, block counts, tables, plane offsets).  Everything else
 * returns -4 (unsupported: the caller falls back to Pillow) before a coefficient is written, a malformed stream -5.  Device half,
 * all images of a call in one launch (at most 32 images per call), a workgroup per tile of 14 x 2 MCUs: dequantisation + libjpeg's
 * accurate integer inverse DCT ("islow") into uint8 component tiles in LDS, then libjpeg-turbo's "fancy" chroma upsampling, YCbCr ->
 * RGB in 16-bit fixed point and the store into (H, W, 3) uint8 rows with a pitch; no workspace.  The chain is stated in DESIGN.md section 4; yardstick
 * tests/_jpeg_reference.py, held against Pillow 12.2 (libjpeg-turbo) bit for bit."""),
    ("pngdec.hip", """PNG decoding split at the filtered scanlines -- np.asarray(Image.open(path)) of SemanticKITTI's image_2 frames and of
 * A2D2's camera and label images (mopa/data/semantic_kitti/semantic_kitti_dataloader.py:563-566, mopa/data/a2d2/preprocess.py:96-141),
 * Pillow's bits after convert("RGB").  Host half (mopa_amd/pngdec.py, no GPU needed): chunk walk with CRC32, IHDR / PLTE / IDAT /
 * IEND, inflate through the standard library's zlib capped one byte past H * (1 + stride); 8-bit samples, colour types 0 / 2 / 3 /
 * 4 / 6, non-interlaced, sides up to 8192.  Device half, all images of a call in one launch (at most 32 images per call), one
 * workgroup per image: lane = row, the rows of a pass advance as a wavefront with a skew of one pixel (the pixel above by lane
 * shuffle, between waves and passes through LDS), None / Sub / Up / Average / Paeth undone on the bytes of a pixel side by side, and
 * the expansion to RGB (grey replicated, alpha dropped, palette looked up) in the store into (H, W, 3) uint8 rows with a pitch;
 * integer only, no atomics, no workspace, no workgroup waits for another.  The chain is stated in DESIGN.md section 4; yardstick
 * tests/_png_reference.py, held against Pillow 12.2."""),
    ("ground.hip", """Ground estimation on the device, all scans of an iteration per launch: the per-point ground mask that obj_on_road
 * (mopa/data/mixmatch_ss.py:380-388) gets from Patchwork++ on the host and the shipped configs load from g_indices_dir
 * (the preprocess.py of each dataset under mopa/data).  NOT the bits of Patchwork++: the published Patchwork core stated in DESIGN.md section 4 (504 patches
 * in four concentric zones, per patch a plane fitted from the lowest points, uprightness / elevation / flatness tests), float64,
 * deterministic; yardstick tests/_ground_reference.py.  The scans are the segments of one (sum N, cols) array, described by a small
 * device table; no read-back."""),
    ("objects.hip", """Object bank on the device, all scans and all requested classes of a call per launch: the instances that
 * mopa/data/waymo/obj_point_extract.py:89-127 cuts out of labelled scans offline -- per (scan, class) the labels of
 * sklearn.cluster.DBSCAN(eps=4, min_samples=5).fit_predict, exactly (uniform grid of side eps, core flags, lock-free union-find
 * over core-core edges, clusters numbered by their lowest core point, border points to the lowest adjacent cluster), the float32
 * range of every point, per instance (np.unique order: the noise group -1 first) the float64 mean range against max_distance,
 * and the instances' points grouped in row order -- what the datasets' obj_sampling (mopa/data/nuscenes/nuscenes_dataloader.py:249-266,
 * mopa/data/semantic_kitti/semantic_kitti_dataloader.py:404-419) later draws from.  Rows with a non-finite coordinate (sklearn raises
 * on them) are left out and counted.  A fixed number of launches; the caller reads back the three counters once, to size its views;
 * yardstick tests/_objects_reference.py."""),
    ("optim.hip", """Adam on one flat fp32 buffer == torch.optim.Adam as built by mopa/common/solver/build.py:7-21 (yaml BASE_LR 1e-3).
 * Not in the reference (opt-in): mopa_grad_stats = per-parameter and total 2-norm, max |g| and non-finite count of the flat gradient
 * (what torch.nn.utils.clip_grad_norm_ and torch.isfinite would compute, without a host read), mopa_adam_flat_guarded = the same
 * update clipped or skipped by the step record that pass leaves in device memory.
 * The other optimizers that call builds by name (getattr(torch.optim, TYPE); mopa/common/config/base.py:42-70 names SGD with
 * momentum / dampening): mopa_sgd_flat == torch.optim.SGD, mopa_adamw_flat == torch.optim.AdamW, each with its guarded form."""),
]

HEAD = """/* libmopa_hip.so -- C ABI of the MI355X-native MoPA hot path (gfx950 only).
 *
 * GENERATED by mopa_amd/csrc/gen_header.py from the MOPA_API definitions; do not edit by hand.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; `stream` is a hipStream_t;
 *   - plain pointers and sizes only (no torch types); no allocation, no global state, re-entrant per stream;
 *   - scratch memory is passed in (`ws`, `ws_bytes`); the matching *_workspace_bytes() query gives the size;
 *   - return value: 0 = ok, -1 = bad argument / unsupported shape, -2 = workspace too small, -3 = launch failed,
 *     -4 = JPEG stream outside the supported subset, -5 = malformed JPEG stream (jpegdec.hip only);
 *   - features are fp32 row-major [rows][ld] (ld >= C lets a layer address a channel slice of a wider buffer).
 * The reference has no FFI of its own (it is pure Python on torch + sparseconvnet); each group below names the
 * reference call sites whose arithmetic it replaces.  Binding example: INTEGRATION.md (ctypes), mopa_amd/_lib.py.
 */
#ifndef MOPA_HIP_H
#define MOPA_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
"""


RETURNS = {"int": "i", "size_t": "z"}
SCALARS = {"int": "i", "int32_t": "i", "int64_t": "l", "uint64_t": "u", "size_t": "z", "float": "f", "double": "d"}

Param = collections.namedtuple("Param", "ctype name pointer code")          # code: 'p' for a pointer, else SCALARS[ctype]
Proto = collections.namedtuple("Proto", "file name ret params text")       # text: the definition's head on one line


def parse(fname):
    """The MOPA_API definitions of one source file, in source order."""
    out = []
    for m in re.finditer(r"MOPA_API\s+([^{;]+?)\s*\{", open(os.path.join(HERE, fname)).read(), re.S):
        text = " ".join(m.group(1).split())
        ret, name, plist = re.match(r"(\w[\w\s\*]*?)\s*(mopa_\w+)\((.*)\)$", text).groups()
        if ret not in RETURNS:
            raise ValueError(f"{fname}: {name} returns `{ret}`; known return types: {', '.join(RETURNS)}")
        params = []
        for prm in re.sub(r"/\*.*?\*/", "", plist).split(","):
            prm = prm.strip()
            if prm in ("", "void"):
                continue
            pname = re.split(r"[\s\*]+", prm)[-1]
            ctype = prm[:len(prm) - len(pname)].strip()
            pointer = "*" in ctype
            scalar = re.sub(r"\bconst\b", "", ctype).strip()
            if not pointer and scalar not in SCALARS:
                raise ValueError(f"{fname}: {name}: parameter `{prm}` has the scalar type `{scalar}`; known: {', '.join(SCALARS)}")
            params.append(Param(ctype, pname, pointer, "p" if pointer else SCALARS[scalar]))
        out.append(Proto(fname, name, ret, params, text))
    return out


def gen_header(protos):
    parts = [HEAD]
    for fname, doc in SECTIONS:
        parts.append(f"\n/* ---- {fname}\n * {doc}\n */")
        parts += [p.text + ";" for p in protos if p.file == fname]
    parts.append("\n#ifdef __cplusplus\n}\n#endif\n#endif /* MOPA_HIP_H */\n")
    return "\n".join(parts)


def gen_exec_table(protos):
    """One `case` per launching entry point (returns int, last parameter `void* stream`) for the command-list executor of
    exec2d.hip -- arguments arrive as 64-bit slots (integers and pointers as int64, float / double as the bit pattern of a double)
    and are cast back to the prototype's types.  Ids are positions in the sorted name list (mopa_exec_fn_id)."""
    fns = sorted((p.name, p.params) for p in protos if p.file != "exec2d.hip" and p.ret == "int" and p.params
                 and (p.params[-1].ctype, p.params[-1].name) == ("void*", "stream"))
    lines = ["// GENERATED by gen_header.py::gen_exec_table from the MOPA_API prototypes; do not edit by hand.",
             "static const char* const EXEC_NAMES[] = {"]
    lines += [f'  "{n}",' for n, _ in fns]
    lines += ["};", f"static const int EXEC_N = {len(fns)};",
              "static int exec_dispatch(int id, const int64_t* a, int nargs) {", "  switch (id) {"]
    for i, (n, params) in enumerate(fns):
        args = []
        for j, prm in enumerate(params):
            if prm.pointer:
                args.append(f"({prm.ctype})(uintptr_t)a[{j}]")
            elif prm.code in "fd":
                args.append(f"({prm.ctype})slot_f(a[{j}])")
            else:
                args.append(f"({prm.ctype})a[{j}]")
        lines.append(f"    case {i}: return nargs == {len(params)} ? {n}({', '.join(args)}) : MOPA_ERR_ARG;")
    lines += ["    default: return MOPA_ERR_ARG;", "  }", "}", ""]
    return "\n".join(lines)


def gen_abi(protos):
    """The ctypes table of mopa_amd/_lib.py, and for every entry point the positions and names of its HOST-pointer parameters
    (names ending in `_host`).  The command-list recorder (mopa_amd/_lib.py::CommandList) copies those it knows the size of into
    its own blob and refuses to record an entry point with any other one -- a recorded raw host address would dangle at replay."""
    lines = ['"""GENERATED by csrc/gen_header.py from the MOPA_API definitions; do not edit by hand.',
             "SIGNATURES: entry point -> (return code, argument codes): 'p' pointer, 'i' int / int32_t, 'l' int64_t, 'u' uint64_t,",
             "'z' size_t, 'f' float, 'd' double.",
             'HOST_PARAMS: entry point -> {argument position: name} of its host-pointer parameters (names ending in _host)."""',
             "SIGNATURES = {"]
    for fname, _ in SECTIONS:
        lines.append(f"    # ---- {fname}")
        lines += [f"    {p.name!r}: ({RETURNS[p.ret]!r}, {''.join(q.code for q in p.params)!r})," for p in protos if p.file == fname]
    lines += ["}", "", "HOST_PARAMS = {"]
    for p in sorted(protos, key=lambda p: p.name):
        host = {j: q.name for j, q in enumerate(p.params) if q.pointer and q.name.endswith("_host")}
        if host:
            lines.append(f"    {p.name!r}: {host!r},")
    lines += ["}", ""]
    return "\n".join(lines)


def generate():
    """-> {path relative to the repository root: text} of every generated file."""
    protos = [p for fname, _ in SECTIONS for p in parse(fname)]
    return {"include/mopa_hip.h": gen_header(protos),
            "mopa_amd/csrc/exec_table.inc": gen_exec_table(protos),
            "mopa_amd/_abi.py": gen_abi(protos)}


def main():
    for path, text in generate().items():
        with open(os.path.join(ROOT, path), "w") as f:
            f.write(text)
        print("wrote", path)


if __name__ == "__main__":
    main()
