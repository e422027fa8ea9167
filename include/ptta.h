/* libptta_hip — C ABI of the MI355X-native ProxyTTA test-time-adaptation step (MSG_CHN, NLSPN and CostDCNet backbones).
 *
 * This is the drop-in boundary for the hot path of seobbro/TTA-depth-completion.  The reference
 * has no FFI for this path (it is Python calling ATen); each entry point below names the Python
 * call(s) it replaces, file:line relative to the reference root.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; tensors are the reference's
 *     own layouts: images (N,3,H,W), depth maps (N,1,H,W), embeddings (rows,512), all fp32,
 *     contiguous.  Weights are passed as the reference's state_dict tensors (fp32, NCHW) and are
 *     re-packed internally.
 *   - all work is enqueued on the hipStream_t argument (pass torch.cuda.current_stream()); nothing
 *     is allocated after ptta_create and no call on the path synchronises (host constants travel as
 *     kernel arguments).  The only calls that wait for the stream are the ones that RETURN a host
 *     value (ptta_get_adam_step, ptta_profile_read), the ones that destroy a captured graph
 *     (option "graph" = 1 only; they wait for its last replay: ptta_load_weights, ptta_bind_adapted, ptta_set_image_norm,
 *     ptta_set_graph(0), a changed max_input_depth in ptta_set_hparams), ptta_step_pipelined when it
 *     is handed a frame it was NOT told about by the previous call (it waits for its own prefix
 *     stream once before computing that frame's prefix in line; an announced frame costs no wait),
 *     and any other entry point called while a prefix is in flight (it waits for the prefix stream).
 *   - return value 0 = ok, <0 = error; ptta_last_error() returns a message.  Nothing is printed.
 *   - one handle per (process, GPU); a handle is not thread-safe.
 */
#ifndef PTTA_H
#define PTTA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ptta_ctx* ptta_handle;
typedef void* ptta_stream;              /* hipStream_t */

/* PTTA_BACKBONE_NLSPN: ExternalModel_Adapt(model_name='nlspn') -- src/nlspn_model_adapt.py:13-128 ->
 * NLSPNModel_Adapt._rgbd_meta_contrast (external_src/NLSPN/src/model/nlspnmodel_adapt.py:850-944), adapter settings of
 * src/nlspn_model_adapt.py:56-68, adapt_parameters('meta_bn') (:322-337).  meta_mode PTTA_META_1LAYER or PTTA_META_2LAYERS (optionally | PTTA_NLSPN_LEGACY_OFFSET), dtype
 * PTTA_DTYPE_F32, any height and width >= 16 (sizes that are not multiples of 16 follow the reference's ceil-halving encoder
 * maps and decoder crops, nlspnmodel_adapt.py:474-490).  Differences from the MSG_CHN handle: embeddings are (rows, 1024)
 * with rows = n*(H/16)*(W/16); ptta_adapted_count() is 88 (conv1_rgb_meta + every BatchNorm2d weight/bias, in the
 * reference's order) and every one of them must be bound; ptta_load_weights ignores BatchNorm running statistics
 * (dropped by 'meta_bn') and the values of adapted tensors (the bound tensors are read instead);
 * ptta_backward ignores its two output pointers (read the 88 gradients with ptta_get_grad) and ptta_adam_step takes
 * NULL gradients (it uses the internal ones); after ptta_set_graph(h, 1) (or PTTA_GRAPH=1) ptta_step and ptta_forward_eval replay
 * captured hipGraphs from their second call on (default off for these handles: measured no faster than plain launches);
 * ptta_profile returns -38.  meta_mode | PTTA_ADAPT_META_ONLY: adapt_parameters('meta') instead (2 adapted tensors; see that flag).
 * PTTA_META_2LAYERS: conv1_rgb_meta = Res_Conv(48, 256) (nlspnmodel_adapt.py:37-45, :1376-1377: conv 48 -> 256, BatchNorm2d + LeakyReLU,
 * conv 256 -> 48 with bias, BatchNorm2d, + its input), fp32 or PTTA_DTYPE_MIXED.  ptta_adapted_count() is 93: the block's seven tensors
 * first, then every other BatchNorm2d; the reference's list has 97 entries because the block's two BatchNorm2d are listed a second time at
 * its end, and Adam steps them twice per step: ptta_adapted_repeat() is 2 for those four.  Not with PTTA_NLSPN_SYNCBN_ADAPT (-38: that
 * list's repeat structure differs).
 * PTTA_META_NONE: the network without the meta layer, NLSPNModel_Adapt._forward (nlspnmodel_adapt.py:792-848) -- what loss_type 'pretrain'
 * and every string without adapt / selfsup / meta / head run (:502-509, :609-616): conv1_rgb feeds fe1 directly, ONE pass per training
 * forward (no zero-image pass), no heads.  Two handle kinds, fp32 on one rank, both with or without PTTA_NLSPN_LEGACY_OFFSET:
 *   PTTA_META_NONE alone: the BatchNorm-adaptation baseline, adapt_parameters('meta_bn') on a model whose head was never prepared.
 *     ptta_adapted_count() is 86 (gamma / beta of every BatchNorm2d: the 'meta_bn' list without conv1_rgb_meta.*, same order),
 *     ptta_adapted_repeat() 1; batch statistics in train and eval forwards.  ptta_embedding_rows() is 0: ptta_forward_train writes the depth
 *     only (emb_out / ref_out must be NULL, -22 otherwise); ptta_step, ptta_loss_forward and ptta_loss_backward run with emb = ref = NULL and
 *     loss_info[3] is exactly 0; ptta_backward takes grad_ref = NULL.  Activations are allocated for n frames, not 2 n.
 *   PTTA_META_NONE | PTTA_ADAPT_META_ONLY: the source model, the loaded checkpoint before any adaptation.  ptta_adapted_count() is 0;
 *     ptta_forward_eval normalises every BatchNorm2d with the LOADED running statistics, in the convolution epilogue as on every
 *     PTTA_ADAPT_META_ONLY handle (option "eval_bn_fused"; a missing buffer: -3 at the first eval forward, naming it).  ptta_forward_train,
 *     ptta_step, ptta_backward and ptta_adam_step return -38 and leave the handle usable.
 *   Both: ptta_load_weights accepts and ignores conv1_rgb_meta.*, proj* and pred* keys (a stage-3 checkpoint holds them); ptta_head_*,
 *     ptta_set_stat_sync, ptta_set_stat_sync_rccl and ptta_set_grad_sync_rccl return -38.  Refused at ptta_create with -38 (reason:
 *     ptta_last_error(NULL)): another backbone, PTTA_DTYPE_MIXED (no bound measured), PTTA_NLSPN_SYNCBN_ADAPT (no heads to append). */
/* PTTA_BACKBONE_COSTDCNET: ExternalModel_Adapt(model_name='costdcnet') -- src/costdcnet_model_adapt.py:31-114 ->
 * CostDCNet._rgbd_meta_contrast (external_src/costdcnet/CostDCNet_adapt.py:207-256), res = 16 planes, up_scale = 4
 * (src/costdcnet_model_adapt.py:47-52), adapt_parameters('meta_bn') (:357-378).  meta_mode PTTA_META_1LAYER or PTTA_META_2LAYERS, dtype
 * PTTA_DTYPE_F32, hp.max_predict_depth > 0 (the far plane).  Shapes not divisible by 16 run the reference's dual-corner
 * padding (:134-210).  Embeddings are (rows, 512) with rows = n'*(H'/32)*(W'/32) over the padded batch / size;
 * ptta_adapted_count() is 32 (conv1_rgb_meta + every BatchNorm2d weight/bias of Encoder2D, the reference's order);
 * ptta_load_weights BINDS the running statistics of BatchNorm3d / BatchNorm1d / the sparse encoder's BatchNorm
 * (updated in place by training forwards, read by the eval forward) and ignores those of BatchNorm2d (dropped by
 * 'meta_bn'); the other remarks of PTTA_BACKBONE_NLSPN apply.
 * meta_mode | PTTA_SYNCBN_ADAPT: the adapted set of the reference's DDP run (src/tta_main.py:326 convert_syncbn() BEFORE :339
 * adapt_parameters): EVERY BatchNorm of the model -- Encoder2D's, the BatchNorm1d inside the sparse encoder's nine MinkowskiBatchNorm
 * (`enc3d.<layer>.bn.weight/bias`), UNet3D's 28 BatchNorm3d, the heads' three BatchNorm1d -- is adapted and has lost its running
 * statistics (batch statistics in train AND eval mode; ptta_load_weights ignores every running_* key).  ptta_adapted_count() is 112
 * unique tensors in the reference's order; the reference's list has 116 entries because enc2d.layer{2,3}.0.norm3.{weight,bias} sit
 * behind two SyncBatchNorm modules (norm3 and downsample[1]) and are listed -- and updated by Adam -- twice per step:
 * ptta_adapted_repeat() is 2 for them, 0 for proj.1 / pred.1 (listed, never given a gradient), 1 otherwise.
 * PTTA_META_2LAYERS: conv1_rgb_meta = Res_Conv(16, 64) (CostDCNet_adapt.py:555-563, :501-502), fp32 only (PTTA_DTYPE_MIXED stays -38 as for
 * the 1layer conv).  ptta_adapted_count() is 37, the reference's list 41 entries: the block's two BatchNorm2d come a second time at its
 * end (ptta_adapted_repeat() 2).  Not with PTTA_SYNCBN_ADAPT (-38). */
enum { PTTA_BACKBONE_MSG_CHN = 0, PTTA_BACKBONE_NLSPN = 1, PTTA_BACKBONE_COSTDCNET = 2 };
/* Storage / arithmetic of the MSG_CHN step.
 * PTTA_DTYPE_F32: every 32-channel map fp32, every product fp32-faithful on the bf16 matrix cores (bf16x3 split, fp32 accumulate).
 * PTTA_DTYPE_MIXED (BASELINE config 2; replaces the all-bf16 mode of rounds 1-4, which missed the tolerance by 9x and is gone): the REAL
 *   frames' forward -- the tensors the scored depth map is made of -- exactly as PTTA_DTYPE_F32; the tensors the reference computes under
 *   no_grad or detaches (the zero-image proxy pass, network_exp_msg_chn_adapt.py:509-532, the embedding branch :551-554) and the data
 *   gradients of loss.backward() (src/tta_main.py:632), which reach the scored depth only through an lr-sized Adam move, are NARROW: bf16
 *   storage, one bf16 MFMA per product, fp32 accumulate -- except the WEIGHT operand of the data gradients, which stays bf16 hi + lo (two
 *   MFMAs, option "bwd_w2"): a rounded weight is a systematic error of the gradient's direction and showed over 100+ steps.  depth_train is bit-identical to PTTA_DTYPE_F32; measured budget per tensor
 *   class: profiles/r05_precision_budget.txt; bounds per mode: tests/test_gpu_mixed.py.  PTTA_ARITH=exact / PTTA_CONV_IMPL=naive are
 *   PTTA_DTYPE_F32-only (ptta_create returns -38 with PTTA_DTYPE_MIXED). */
/* PTTA_BACKBONE_NLSPN with PTTA_DTYPE_MIXED: the generic engine keeps fp32 storage and switches the matrix-core convolutions of the proxy
 * frames to one bf16 MFMA per product and those of the data gradients to two (hi activations x hi + lo weights; PTTA_MIXED_BWD_ROUNDED_W:
 * one, round 5's form -- scored depth 2.0e-4 after config 3's three steps and growing 6e-5 per step with it).
 * PTTA_BACKBONE_COSTDCNET refuses it (-38): its scored depth leaves the tolerance (profiles/r06_nlspn_costdcnet_mixed.txt). */
enum { PTTA_DTYPE_F32 = 0, PTTA_DTYPE_MIXED = 1,
       /* OR-ed into PTTA_DTYPE_MIXED (precision budget, tools/accuracy_report.py --keep): keep one of the three narrow classes at fp32 storage
        * and bf16x3 arithmetic -- the proxy chain, the data gradients, the heads */
       PTTA_MIXED_KEEP_PROXY = 0x100, PTTA_MIXED_KEEP_BACKWARD = 0x200, PTTA_MIXED_KEEP_HEADS = 0x400,
       /* generic engine, comparison only: the data gradients on bf16-ROUNDED weights, one MFMA per product (round 5's mixed mode) */
       PTTA_MIXED_BWD_ROUNDED_W = 0x800 };
/* conv1_rgb_meta = Conv2d(32,32,3) | Res_Conv(32,128) (NLSPN: 48 / 256, CostDCNet: 16 / 64) | no meta layer at all (NLSPN only: the source
 * model and the BatchNorm-adaptation baseline, see PTTA_BACKBONE_NLSPN) */
enum { PTTA_META_1LAYER = 0, PTTA_META_2LAYERS = 1, PTTA_META_NONE = 2 };
/* NLSPN only, OR-ed into meta_mode: ExternalModel_Adapt(..., offset=True) -> args.legacy (src/nlspn_model_adapt.py:62):
 * the confidence gathers add each tap's own (dy, dx) to the learned offset (nlspnmodel_adapt.py:297-302).
 * src/tta_main.py:309-317 always constructs the model this way. */
enum { PTTA_NLSPN_LEGACY_OFFSET = 0x100,
       /* NLSPN, OR-ed into meta_mode: the adapted list of the reference's DDP run.  tta_main.py:326 converts every BatchNorm to
        * SyncBatchNorm BEFORE adapt_parameters('meta_bn') (:339), whose isinstance test (src/nlspn_model_adapt.py:329-331) then
        * also matches the heads' three BatchNorm1d: 94 adapted tensors (proj.1, proj_t.1, pred.1 weight/bias appended in
        * module order) instead of 88.  proj / pred feed the detached embedding: their gradients stay zero. */
       PTTA_NLSPN_SYNCBN_ADAPT = 0x200,
       PTTA_SYNCBN_ADAPT = 0x200,          /* the same switch for PTTA_BACKBONE_COSTDCNET (see there) */
       /* NLSPN, OR-ed into meta_mode: the reference's adapt_mode 'meta' (and 'meta_fix': the same optimiser list, numerically identical in one
        * process), src/nlspn_model_adapt.py:302-320 -- the method itself: the meta layer alone adapts, every BatchNorm2d is frozen.
        * ptta_adapted_count() is 2: conv1_rgb_meta.weight, conv1_rgb_meta.bias.  'meta' keeps the loaded running statistics and only sets
        * track_running_stats = False, so BatchNorm2d behaves differently from 'meta_bn' (which drops the buffers): train-mode passes (the
        * grad pass and the proxy pass of ptta_forward_train / ptta_step) normalise with batch statistics and write NO buffer; ptta_forward_eval,
        * the scored forward (src/tta_main.py:729-736), normalises every BatchNorm2d with the LOADED running statistics and loaded gamma / beta:
        * a constant per-channel affine, which runs in the epilogue of the convolution in front of it (option "eval_bn_fused") -- no statistics,
        * finalize or apply pass in that forward.  The backward sweep computes no gamma / beta gradient and no weight gradient but the meta
        * conv's; it still carries the BatchNorm data gradient.  ptta_load_weights keeps running_mean / running_var of every BatchNorm2d; a state
        * dict without them loads, and the first ptta_forward_eval returns -3 naming the missing tensor.  ptta_debug_tensor reads them back
        * by their state-dict names ("conv2.0.bn1.running_var", ".weight", ...).  The heads' BatchNorm1d are as in 'meta_bn' (train mode on the
        * TTA path, their bound buffers updated; no part of the eval forward).
        * Refused with -38 (ptta_last_error with a NULL handle holds the reason): another backbone; PTTA_META_2LAYERS (the reference freezes the
        * block's own BatchNorm2d while still listing its gamma / beta: separate work); PTTA_DTYPE_MIXED (no bound measured);
        * PTTA_NLSPN_SYNCBN_ADAPT.  On such a handle ptta_set_stat_sync, ptta_set_stat_sync_rccl and ptta_set_grad_sync_rccl return -38 and leave it
        * unchanged (one rank only). */
       PTTA_ADAPT_META_ONLY = 0x400,
       /* CostDCNet, OR-ed into PTTA_META_1LAYER: the network without the meta layer, CostDCNet._forward (external_src/costdcnet/CostDCNet_adapt.py:
        * 177-205) -- what loss_type 'pretrain' (the reference's default) runs: Encoder2D -> fusion -> UNet3D -> regression, no conv1_rgb_meta, no
        * zero-image pass, no heads (ptta_embedding_rows() is 0).  fp32, one rank.  (PTTA_META_NONE with PTTA_BACKBONE_COSTDCNET stays refused.)
        *   PTTA_COSTDC_PLAIN | PTTA_ADAPT_META_ONLY: the source model, the loaded checkpoint before any adaptation.  ptta_adapted_count() is 0;
        *     ptta_forward_eval only: EVERY BatchNorm normalises with its loaded running statistics -- Encoder2D's 15 BatchNorm2d (kept by
        *     ptta_load_weights on this handle) and the UNet3D's 28 BatchNorm3d + ELU as constant affines in the epilogues of the convolutions in
        *     front of them (option "eval_bn_fused", default 1; "eval_bn_fused_count" reads 43), the sparse encoder's nine as their own launches.
        *     The tables are built once per load; a state dict without one of the buffers loads, and the first ptta_forward_eval returns -3 naming
        *     the missing tensor.  ptta_load_weights accepts and ignores conv1_rgb_meta.*, proj* and pred* (a stage-3 checkpoint holds them).
        *     ptta_forward_train, ptta_step, ptta_backward and ptta_adam_step return -38 and leave the handle usable; so do ptta_head_* and the
        *     three exchange setters.  The dual-corner padding works as on the ProxyTTA handle.
        *   PTTA_COSTDC_PLAIN alone: the BatchNorm-adaptation baseline, adapt_parameters('meta_bn') on a model whose head was never prepared
        *     (src/costdcnet_model_adapt.py:357-378).  ptta_adapted_count() is 30: gamma / beta of Encoder2D's 15 BatchNorm2d in the order of the
        *     32-entry list minus conv1_rgb_meta.*; ptta_adapted_repeat() is 1.  A training forward is ONE pass: emb_out, ref_out of
        *     ptta_forward_train and grad_ref of ptta_backward must be NULL, loss_info[3] is exactly 0, and activations are allocated for n frames,
        *     not 2 n.  BatchNorm2d uses batch statistics in train and eval forwards (its running statistics are dropped); BatchNorm3d and the
        *     sparse encoder's BatchNorm use batch statistics in train mode and update their bound running statistics ONCE per training forward
        *     (num_batches_tracked + 1, where the ProxyTTA handle's two passes add 2), and use them in eval.  "eval_bn_fused" is -38 (no constant
        *     affine).  ptta_head_* and the three exchange setters return -38.
        * Refused with -38 and a reason in ptta_last_error(NULL): another backbone, PTTA_META_2LAYERS, PTTA_SYNCBN_ADAPT, PTTA_DTYPE_MIXED. */
       PTTA_COSTDC_PLAIN = 0x800 };
/* MSG_CHN, OR-ed into PTTA_META_1LAYER: the source model, network._forward (network_exp_msg_chn_adapt.py:402-403, :418-461) -- what loss_type
 * 'pretrain' (the reference's default) runs, on a prepared model too: the loaded checkpoint without conv1_rgb_meta, without the zero-image
 * pass and without the heads.  The three places that read the meta layer's output (depth_decoder1.dec1.3, depth_decoder2.dec2.3,
 * depth_encoder3.enc2.3) read the RGB encoder's quarter-resolution map instead, and no meta convolution is launched.  fp32, one rank.
 *   ptta_forward_eval only: the depth is `_forward`'s output_d11, the one scale the eval wrapper returns (src/msg_chn_model_adapt.py:179-181).
 *     Sizes not divisible by 16 run the dual-corner padding and the mean of the two crops as on the ProxyTTA handle; ptta_set_image_norm and
 *     the options that select launch forms of the forward ("graph", "pair_fuse", "tpair_fuse", "fuse_first") work.
 *   ptta_adapted_count() and ptta_embedding_rows() are 0.  ptta_forward_train, ptta_step, ptta_step_pipelined, ptta_forward_eval_last,
 *     ptta_pipeline_stream, ptta_backward, ptta_adam_step, ptta_loss_forward, ptta_loss_backward, every ptta_head_* and the three exchange
 *     setters return -38 with a reason and leave the handle usable.  ptta_profile brackets the launches of the eval forward.
 *   Activations are allocated for n frames, not 2 n (ptta_debug_tensor reports the halved sizes; "m" is an unknown name); the narrow copies,
 *     the proxy-RGB constants, the heads' weights and workspace, the backward's 32 -> 32 weight packs, masks and gradient maps, the weight-gradient
 *     partials and the Adam state are not allocated at all.
 *   ptta_load_weights accepts a state dict without conv1_rgb_meta.*, proj* and pred* keys and ignores them when present, in their 1layer
 *     and their 2layers form alike (a stage-3 checkpoint holds them).
 * Refused at ptta_create with -38 and a reason in ptta_last_error(NULL): another backbone, PTTA_META_2LAYERS or PTTA_META_NONE as the base
 * mode, PTTA_DTYPE_MIXED (the scored forward of the mixed mode is the fp32 one already), any other flag beside it. */
enum { PTTA_MSGCHN_PLAIN = 0x1000 };

/* Hyper-parameters of the step.  Reference: src/tta.py:10-160 flags learning_rates,
 * optimizer_betas, optimizer_epsilon, w_weight_decay, w_loss_sparse_depth, w_loss_smoothness,
 * w_loss_cos, max_input_depth (forwarded positionally to src/tta_main.py:23-100). */
typedef struct {
    float lr, beta1, beta2, eps, weight_decay;
    float w_sparse_depth, w_smoothness, w_cos;
    float max_input_depth;              /* < 0: no clamp (max_input_depth=None) */
    float max_predict_depth;            /* CostDCNet only: ExternalModel_Adapt(max_predict_depth) = far plane of the cost volume */
} ptta_hparams;

/* ExternalModel_Adapt(model_name='msg_chn', ...) + _prepare_head(prepare_mode)
 * (src/external_model_adapt.py:46-80, :561; network_exp_msg_chn_adapt.py:1022-1087).
 * n, height, width: batch and frame size of every later call.  Shapes not divisible by 16 run
 * the reference's dual-corner padding (src/msg_chn_model_adapt.py:60-123) internally. */
int ptta_create(ptta_handle* out, int backbone, int meta_mode, int n, int height, int width, int dtype,
                const ptta_hparams* hp_host);
void ptta_destroy(ptta_handle h);
const char* ptta_last_error(ptta_handle h);

/* optimizer.param_groups[i]['lr'] = ... (src/tta_main.py:507-512) and the loss weights. */
int ptta_set_hparams(ptta_handle h, const ptta_hparams* hp_host, ptta_stream s);

/* restore_model -> load_state_dict(checkpoint['net']) (src/msg_chn_model_adapt.py:482-501), one
 * call per state_dict key.  Frozen tensors are copied and re-packed; BatchNorm buffers
 * (*.running_mean / *.running_var / *.num_batches_tracked) are BOUND: the pointer is kept and
 * updated in place by every training-mode forward, as nn.BatchNorm1d does.  Unknown keys: error. */
int ptta_load_weights(ptta_handle h, const char* name, const void* tensor, const int64_t* shape, int ndim,
                      ptta_stream s);

/* adapt_parameters(mode='meta') + torch.optim.Adam state (src/msg_chn_model_adapt.py:392-396,
 * src/tta_main.py:339-346).  The caller keeps ownership of the parameter and of the Adam moments
 * exp_avg / exp_avg_sq (fp32, same shape); the library reads the parameter on every forward and
 * ptta_step / ptta_adam_step update all three in place.  name: one of ptta_adapted_name(). */
int ptta_bind_adapted(ptta_handle h, const char* name, float* param, float* exp_avg, float* exp_avg_sq);
int ptta_set_adam_step(ptta_handle h, int step, ptta_stream s);      /* optimizer.state[p]['step'] */
int ptta_get_adam_step(ptta_handle h, int* step_host, ptta_stream s); /* synchronises s */

/* model.train(); model.forward(image, sparse_depth, loss_type='adapt_meta_selfsup_seq_ema_reverse')
 * (src/tta_main.py:610 -> external_model_adapt.py:82-114 -> msg_chn_model_adapt.py:54-125 ->
 * network_exp_msg_chn_adapt.py:463-557).  Outputs: depth (N,1,H,W), emb/ref (rows,512) with
 * rows = ptta_embedding_rows(h).  Activations needed by ptta_backward stay in the handle. */
int ptta_forward_train(ptta_handle h, const float* image, const float* sparse_depth,
                       float* depth_out, float* emb_out, float* ref_out, ptta_stream s);
int64_t ptta_embedding_rows(ptta_handle h);

/* model.eval(); with no_grad: model.forward(...) (src/tta_main.py:729-736). */
int ptta_forward_eval(ptta_handle h, const float* image, const float* sparse_depth, float* depth_out, ptta_stream s);

/* model.compute_loss(..., loss_type='adapt') (src/external_model_adapt.py:119-203, :371-441).
 * loss_info_out[4] (device) = {loss, loss_smooth, loss_sparse_depth, loss_cos}.  emb/ref may be
 * NULL (loss_cos = 0).  The backward half writes dL/d(depth) (N,1,H,W) and dL/d(ref) (rows,512). */
int ptta_loss_forward(ptta_handle h, const float* loss_image, const float* depth, const float* sparse_depth,
                      const float* validity, const float* emb, const float* ref, int64_t rows,
                      float w_sparse_depth, float w_smoothness, float w_cos, float* loss_info_out, ptta_stream s);
int ptta_loss_backward(ptta_handle h, const float* loss_image, const float* depth, const float* sparse_depth,
                       const float* validity, const float* emb, const float* ref, int64_t rows,
                       float* grad_depth_out, float* grad_ref_out, ptta_stream s);

/* loss.backward() restricted to the adapted parameters (src/tta_main.py:632): consumes
 * dL/d(depth) and dL/d(ref) of the last ptta_forward_train and writes the gradients of
 * conv1_rgb_meta.{weight (32,32,3,3), bias (32)}. */
int ptta_backward(ptta_handle h, const float* grad_depth, const float* grad_ref,
                  float* grad_meta_weight_out, float* grad_meta_bias_out, ptta_stream s);

/* Gradient of one adapted parameter after ptta_backward / ptta_step, by state_dict key (the
 * 2layers meta layer has seven adapted tensors: two conv weights, one conv bias, two BatchNorm
 * gamma/beta pairs).  ptta_adapted_count/name enumerate them in state_dict order. */
int ptta_get_grad(ptta_handle h, const char* name, float* dst, int64_t capacity, ptta_stream s);
/* Overwrite the stored gradient of one adapted parameter (e.g. with the mean over ranks that DistributedDataParallel
 * would have produced, src/msg_chn_model_adapt.py:476-480) before ptta_adam_step(h, NULL, NULL, s). */
int ptta_set_grad(ptta_handle h, const char* name, const float* src, int64_t numel, ptta_stream s);
int ptta_adapted_count(ptta_handle h);
const char* ptta_adapted_name(ptta_handle h, int index, int64_t* numel_host);
/* How many times the reference's parameter list names this tensor = the Adam updates it receives per optimizer.step()
 * (torch.optim.Adam walks the list; a tensor listed twice is stepped twice with the same gradient).  1 except under PTTA_SYNCBN_ADAPT and
 * under PTTA_META_2LAYERS on NLSPN / CostDCNet (see those backbones). */
int ptta_adapted_repeat(ptta_handle h, int index);

/* ptta_step for a STREAM of frames (MSG_CHN handles; others forward to ptta_step): besides the step on (image, sparse) it starts, on a stream
 * of its own, the part of the NEXT frame's forward that does not depend on the adapted parameters -- clamp / pooling of the sparse depth, the
 * frozen RGB encoder, the depth-only head of the stage-1 encoder (everything upstream of conv1_rgb_meta) -- so that it runs beside this
 * frame's step instead of at the head of the next one.  Results are those of ptta_step, call by call (the prefix's outputs exist twice).
 * Frames are named by TOKENS the caller chooses: non-zero, and a NEW one whenever the frame CONTENT is new (a counter).  next_image /
 * next_sparse / next_token: the frame the FOLLOWING call will pass as (image, sparse, frame_token); it is copied into the handle when it is
 * announced, so the caller's buffers only have to hold it until this call's work on the prefix stream has run.  The prepared prefix is used
 * iff the following call's frame_token equals the announced next_token -- never by pointer identity: refilling one staging buffer with another
 * frame is safe as long as the new content gets a new token (tests/test_gpu_staging_augment.py).  next_token == frame_token: another step
 * on the same frame (inner_iter > 1), its prefix is kept.  A token of 0 = unnamed: frame_token 0 never matches (prefix computed in line),
 * next_token 0 / NULL pointers prepare nothing.  The reference's loop knows its next frame from the data loader (src/tta_main.py:519-523).
 * ptta_forward_eval / ptta_forward_train between two calls are fine (they run in, and invalidate, the buffer set of the last processed frame).
 * Host synchronisation: none when the frame was announced; an UNANNOUNCED frame (first call, token mismatch) waits for the prefix stream
 * on the host once before computing its prefix in line. */
int ptta_step_pipelined(ptta_handle h, const float* image, const float* loss_image, const float* sparse_depth, const float* validity_map,
                        uint64_t frame_token, const float* next_image, const float* next_sparse_depth, uint64_t next_token,
                        float* depth_out, float* loss_info_out, ptta_stream s);
/* The stream the next frame's prefix runs on: when that frame is still arriving (an asynchronous H2D copy), make THIS stream wait for the
 * copy's event before the call that announces the frame -- not the caller's stream, which would delay the current step. */
int ptta_pipeline_stream(ptta_handle h, ptta_stream* stream_out);
/* The scored eval forward (src/tta_main.py:729-736) of the frame the last ptta_step_pipelined call adapted, without recomputing that
 * frame's parameter-independent prefix (it is still in the handle).  When that call ran as a plain ptta_step (profiling, validation kernels,
 * SyncBatchNorm / gradient exchange, padded sizes) this is a full ptta_forward_eval of its frame, read from the caller's
 * buffers of that call (which must still hold it).  -3 when no such frame is held (e.g. after ptta_load_weights or a ptta_forward_eval). */
int ptta_forward_eval_last(ptta_handle h, float* depth_out, ptta_stream s);

/* optimizer.step() for the bound parameters with explicit gradients (src/tta_main.py:633). */
int ptta_adam_step(ptta_handle h, const float* grad_meta_weight, const float* grad_meta_bias, ptta_stream s);

/* One whole TTA step = src/tta_main.py:610-633: forward_train + compute_loss + zero_grad +
 * backward + optimizer.step, in one enqueue.  `image` feeds the network, `loss_image` the
 * smoothness weights (tta_main.py:610 vs :620; may be the same pointer).  validity NULL =>
 * where(sparse>0,1,sparse) (tta_main.py:583-586).  Optional outputs may be NULL. */
int ptta_step(ptta_handle h, const float* image, const float* loss_image, const float* sparse_depth,
              const float* validity, float* depth_out, float* loss_info_out, ptta_stream s);

/* OutlierRemoval(kernel_size, threshold).remove_outliers(sparse_depth, validity_map) (src/net_utils.py:750-811),
 * the on-device filter src/tta_main.py:590 applies before every forward.  Handle-free; scratch = 4 KiB of
 * device memory (1024 floats).  Outputs may not alias the inputs. */
int ptta_outlier_removal(const float* sparse_depth, const float* validity, float* sparse_out, float* validity_out,
                         int n, int height, int width, int kernel_size, float threshold, float* scratch, ptta_stream s);

/* Validation metrics of src/tta_main.py:779-798 (eval_utils.py:117-174) reduced on device:
 * metrics_out[4] (device) = {MAE mm, RMSE mm, iMAE 1/km, iRMSE 1/km} over pixels with ground_truth > 0 and
 * min <= ground_truth <= max.  scratch: 16 KiB of device memory.  Handle-free. */
int ptta_eval_metrics(const float* depth, const float* ground_truth, int64_t numel, float min_evaluate_depth,
                      float max_evaluate_depth, void* scratch, float* metrics_out, ptta_stream s);

/* The reference's native extension `DCN` (external_src/NLSPN/src/model/deformconv/src/vision.cpp:7-12):
 *   modulated_deform_conv_forward(input, weight, bias, offset, mask, kh,kw, sh,sw, ph,pw, dh,dw, group,
 *                                 deformable_group, im2col_step) -> output           (modulated_deform_conv.h:10-26)
 *   modulated_deform_conv_backward(..., grad_output, ...) -> [grad_input, grad_offset, grad_mask, grad_weight, grad_bias]
 *                                                                                     (modulated_deform_conv.h:46-63)
 * NCHW fp32 contiguous, offset (B, 2*K*dg, Ho, Wo), mask (B, K*dg, Ho, Wo).  im2col_step has no meaning here (no
 * column buffer).  bias may be NULL; any grad_* pointer may be NULL.  Handle-free. */
int ptta_mdconv_forward(const float* input, const float* weight, const float* bias, const float* offset, const float* mask,
                        float* output, int b, int c, int h, int w, int c_out, int kh, int kw, int sh, int sw, int ph, int pw,
                        int dh, int dw, int group, int deformable_group, ptta_stream s);
int ptta_mdconv_backward(const float* input, const float* weight, const float* bias, const float* offset, const float* mask,
                         const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                         float* grad_bias, int b, int c, int h, int w, int c_out, int kh, int kw, int sh, int sw, int ph, int pw,
                         int dh, int dw, int group, int deformable_group, ptta_stream s);

/* Photometric normalisation of the network input, fused into the first convolution's loads (and into
 * the dual-corner padding): replaces Transforms.normalize_images (src/transforms.py:668-710) as called at
 * src/tta_main.py:454-464,652 -- image -> (image / divisor - mean[c]) / std[c].  [0,1] is (255, 0, 1);
 * [-1,1] is (255, .5, .5); standard normalisation is (255, mean, std).  After this call `image` in
 * ptta_forward_train / ptta_forward_eval / ptta_step is the RAW image; the loss keeps using the raw image
 * unless a separate loss_image is passed, which is what the reference does (tta_main.py:610,620).
 * mean / std may be NULL (0 / 1).  (1, 0, 1) switches it off. */
int ptta_set_image_norm(ptta_handle h, float divisor, const float* mean, const float* stdv);

/* ---- Stage-2 head trainer ------------------------------------------------------------------------------
 * One step of src/head_main.py:464-480 for MSG_CHN (fp32 handle, sizes divisible by 16) with loss_type
 * 'head_selfsup_seq_ema_reverse' (reverse = 1) or 'head_selfsup_seq_ema' (reverse = 0), i.e.
 * network_exp_msg_chn_adapt.py:610-699 (`_rgbd_meta_contrast_head`, mode without 'adapt'):
 *   _update_head()           proj_t <- tau proj_t + (1 - tau) proj over parameters()                    (:701-703)
 *   both backbone passes     no gradient, train-mode BatchNorm, stop at depth_encoder3                      (:626-676)
 *   reverse:     emb = pred(proj(feat_zero).detach()), ref = proj(feat).detach()      -> pred trains      (:691-694)
 *   not reverse: emb = pred(proj(feat)),               ref = proj(feat_zero).detach() -> proj, pred train (:681-684)
 *   prepare_loss             mean(2 - 2 <normalize(emb), normalize(ref)>)          (src/external_model_adapt.py:524-541)
 *   Adam                     over prepare_parameters('head_selfsup_ema') (src/msg_chn_model_adapt.py:297-304); parameters
 *                            without a gradient are skipped like torch.optim.Adam skips .grad == None
 * NLSPN and CostDCNet handles (csrc/ghead.hip; nlspnmodel_adapt.py:1014-1060, CostDCNet_adapt.py:258-303): the same calls.  There the reference branch
 * goes through the EMA target -- not reverse: emb = pred(proj(rows(real).detach())), ref = proj_t(rows(zero image)).detach(); reverse: the passes
 * swapped -- so proj AND pred train in both directions (ptta_head_get_grad: has_grad = 1 for all twelve), proj_t's BatchNorm1d runs in train mode
 * like the other two, and the backbone's BatchNorm2d layers normalise with their LOADED running statistics (`train(prepare=True)`,
 * src/nlspn_model_adapt.py:360-368, src/costdcnet_model_adapt.py:418-430) -- ptta_load_weights keeps them for this purpose; BatchNorm3d and the
 * sparse encoder's BatchNorm1d stay in train mode as in the reference.  Not offered (-38) with PTTA_SYNCBN_ADAPT, a statistics exchange of
 * more than one rank in the plain form (ptta_head_set_form), or (CostDCNet) sizes that need the dual-corner padding.
 * ptta_head_bind: name in {proj,pred}.{0,3}.{weight,bias}, {proj,pred}.1.{weight,bias} (param + both Adam moments, device fp32,
 * caller-owned, updated in place) or proj_t.* (param only; bind all six or none).  After ptta_head_adam_step the handle's
 * packed copies of the updated head weights are re-derived, so TTA calls on the same handle see them; after an EXTERNAL
 * update of bound parameters call ptta_head_reload.  adam_step < 0 in ptta_head_set_hparams keeps the device-side count.
 * ptta_head_step = forward + backward + adam_step.  loss_out: 1 device float.  Everything enqueues only. */
int ptta_head_bind(ptta_handle h, const char* name, float* param, float* exp_avg, float* exp_avg_sq);
int ptta_head_set_hparams(ptta_handle h, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                          int adam_step, ptta_stream s);
int ptta_head_reload(ptta_handle h, ptta_stream s);
int ptta_head_forward(ptta_handle h, const float* image, const float* sparse_depth, int reverse, float* emb_out, float* ref_out,
                      ptta_stream s);
int ptta_head_backward(ptta_handle h, float* loss_out, ptta_stream s);
int ptta_head_adam_step(ptta_handle h, ptta_stream s);
int ptta_head_step(ptta_handle h, const float* image, const float* sparse_depth, int reverse, float* loss_out, ptta_stream s);
/* gradient of the last ptta_head_backward; *has_grad_host = 0 (and dst untouched) for parameters outside the graph */
int ptta_head_get_grad(ptta_handle h, const char* name, float* dst, int64_t capacity, int* has_grad_host, ptta_stream s);

/* SyncBatchNorm form of the stage-2 head trainer: what the reference's stage 2 always runs.  src/head_main.py:278 convert_syncbn() and :279
 * distributed_data_parallel(rank) run before train(prepare=True) (:407, :417), and src/train_head.py:178 spawns one rank per visible GPU.
 * PTTA_HEAD_FORM_PLAIN (the default) stays the unconverted single-process form described above.  Under PTTA_HEAD_FORM_SYNCBN:
 *   NLSPN      proj_t.1 (the EMA target's BatchNorm1d) is in eval mode: train_prepare's isinstance test (src/nlspn_model_adapt.py:360-368)
 *              matches SyncBatchNorm, so it normalises with its loaded running statistics and leaves them untouched.
 *   CostDCNet  proj_t.1, UNet3D's BatchNorm3d and the sparse encoder's BatchNorm1d are in eval mode with frozen affine
 *              (src/costdcnet_model_adapt.py:418-430): running statistics bound by ptta_load_weights, untouched.
 *   MSG_CHN    train_prepare is plain train() (src/msg_chn_model_adapt.py:435-440): one rank computes exactly the plain form.
 *   every backbone, stat_sync world > 1 (ptta_set_stat_sync / ptta_set_stat_sync_rccl): proj.1 / pred.1 take the moments of the GLOBAL
 *              batch in the forward and the backward; their running statistics use the global row count.  Before the head Adam the twelve
 *              gradients, one arena, are averaged over the ranks as ONE message: ptta_set_grad_sync_rccl's communicator, or, without one,
 *              the statistics exchange itself (its callback or its communicator) in chunks of its buffer (an fp64 sum, then / world:
 *              bitwise the same on every rank; a buffer of at least the twelve tensors' numel makes it one message).
 * Call before the first ptta_head_forward / ptta_head_step (-3 after it).  Refused (-38) on handles of PTTA_DTYPE_MIXED.  The form does
 * not select the TTA adapted list (PTTA_SYNCBN_ADAPT): it applies to handles built without it.  The plain form returns -38 with world > 1. */
enum { PTTA_HEAD_FORM_PLAIN = 0, PTTA_HEAD_FORM_SYNCBN = 1 };
int ptta_head_set_form(ptta_handle h, int form);

/* Geometric augmentation on device: Transforms.crop + horizontal_flip + vertical_flip
 * (src/transforms.py:337-407, 955-1034) in one pass over an N x C x H x W fp32 tensor:
 *   dst[b,c,y,x] = src[b, c, start_y[b] + (vflip[b] ? ch-1-y : y), start_x[b] + (hflip[b] ? cw-1-x : x)]
 * (the reference crops first and flips the cropped sample).  start_y / start_x (int32, device, per sample; NULL = 0) and
 * hflip / vflip (uint8, device, per sample; NULL = no flip) are the caller's random draws; starts are clamped into the
 * sample.  dst is N x C x crop_height x crop_width and must not alias src.  Handle-free, enqueues only. */
int ptta_crop_flip(const float* src, float* dst, int n, int channels, int height, int width, int crop_height, int crop_width,
                   const int32_t* start_y, const int32_t* start_x, const uint8_t* hflip, const uint8_t* vflip, ptta_stream s);

/* Raw-frame ingest on device: the reference's loader arithmetic and crop in one pass over the frames AS DECODED, so that 5 bytes per pixel
 * cross the host link instead of 16.  image_u8 is N x src_height x src_width x 3 uint8 (a decoded RGB PNG), sparse_u16 / gt_u16 are
 * N x src_height x src_width 16-bit integers (decoded depth PNGs), all on the device:
 *   image_out[b,c,y,x]  = (float) image_u8[b, sy+y, sx+x, c]             load_image(normalize=False, 'CHW'): np.asarray(image, np.float32) +
 *                                                                        np.transpose (src/data_utils.py:150-158, src/datasets.py:399-407)
 *   sparse_out[b,0,y,x] = (float) sparse_u16[b, sy+y, sx+x] / multiplier load_depth (src/data_utils.py:219-223): one IEEE fp32 division
 *   validity_out        = sparse_out > 0 ? 1 : 0                         load_depth_with_validity_map (:182-188)
 *   gt_out, gt_validity_out: the same from gt_u16
 * and [sy : sy+height, sx : sx+width] is the loader's random / bottom crop (src/datasets.py:83-170): start_y / start_x are int32, device,
 * per sample (NULL = 0), the caller's draws, clamped into the sample exactly as ptta_crop_flip clamps them.  Outputs are N x 3 x height x
 * width and N x 1 x height x width fp32.  Each input may be NULL together with its outputs; validity_out and gt_validity_out may be NULL on
 * their own.  -22 before any launch: an output without its input, an input without its output, no input at all, n < 1, a size < 1,
 * height > src_height or width > src_width, a multiplier that is not a positive finite number.  Rows of a width that is a multiple of 4
 * (16-byte-aligned outputs) are written with 16-byte stores; no byte outside the three source arrays is read.  Flips stay with
 * ptta_crop_flip, behind ptta_outlier_removal as the reference orders them.  Handle-free, one launch, enqueues only. */
int ptta_ingest_raw(const uint8_t* image_u8, const uint16_t* sparse_u16, const uint16_t* gt_u16, float* image_out, float* sparse_out,
                    float* validity_out, float* gt_out, float* gt_validity_out, int n, int src_height, int src_width, int height, int width,
                    const int32_t* start_y, const int32_t* start_x, float multiplier, ptta_stream s);

/* Raw-frame egress on device, the inverse of ptta_ingest_raw: the reference's writers' arithmetic and the paste back into the stored frame
 * in one pass, so that 2 bytes per pixel (2 + 2 + 3 with validity and image) cross the host link instead of 4 (4 + 4 + 12).  depth and
 * validity are N x 1 x height x width fp32, image is N x 3 x height x width fp32, all on the device:
 *   depth_u16[b, sy+y, sx+x]    = p > 0 ? (uint16) min(trunc(p), 65535) : 0, p = depth[b,0,y,x] * multiplier (one fp32 multiply)
 *                                                                        save_depth: np.uint32(z * multiplier) as a 16-bit PNG
 *                                                                        (src/data_utils.py:236-251)
 *   validity_u16[b, sy+y, sx+x] = validity[b,0,y,x] > 0 ? 256 : 0        save_validity_map (:283-298)
 *   image_u8[b, sy+y, sx+x, c]  = q > 0 ? (uint8) min(trunc(q), 255) : 0, q = image[b,c,y,x] * image_scale (one fp32 multiply; 255 for
 *                                                                        normalized=True, 1 for False)
 *                                                                        save_image(..., data_format='CHW') (:29-78)
 * Outputs are N x dst_height x dst_width uint16 and N x dst_height x dst_width x 3 uint8, the stored frame; the input lands in the window
 * [sy : sy+height, sx : sx+width] of its sample and every output element outside it is written 0: the caller never clears an output.
 * start_y / start_x are int32, device, per sample (NULL = 0), clamped into the sample exactly as ptta_ingest_raw and ptta_crop_flip clamp
 * them.  Where the reference is defined (0 <= p < 2^31, 0 <= q < 256) the bits are its own: it truncates, and Pillow stores 65535 for
 * everything at or above 65536.  Outside that range its result is an accident of casts and this library defines it: a negative value, -0
 * and NaN give 0; anything at or above the top of the range, +inf included, gives 65535 (255 for the image, where the reference wraps).
 * NaN validity gives 0.  Each input may be NULL together with its output.  -22 before any launch, with the reason in
 * ptta_last_error(NULL): no input at all, an input without its output or an output without its input, n < 1, a size < 1,
 * height > dst_height or width > dst_width, a multiplier or image_scale that is not a positive finite number, an odd depth_u16 or
 * validity_u16 address.  Every output byte is written exactly once, 16-bit rows with 16-byte stores laid on the destination's alignment,
 * and no byte outside the inputs is read; results are bit-identical from run to run.  Handle-free, one launch, enqueues only. */
int ptta_egress_raw(const float* depth, const float* validity, const float* image, uint16_t* depth_u16, uint16_t* validity_u16,
                    uint8_t* image_u8, int n, int height, int width, int dst_height, int dst_width, const int32_t* start_y,
                    const int32_t* start_x, float multiplier, float image_scale, ptta_stream s);

/* Eval-time hole filling on device (src/nlspn_model_adapt.py:124-127; the definition is proxytta/inpaint.py, the scipy restatement of
 * skimage.restoration.inpaint_biharmonic): per sample of the N x 1 x height x width fp32 map `depth`, the exact zeros are the unknowns of
 * the biharmonic system the host code builds (radius-2 box clipped to the image, Laplacian with replicated box edges, known pixels on the
 * right-hand side in fp64); it is solved by conjugate gradients in fp64 from x = 0 until |r| <= rtol |b|, and each hole becomes
 * (float) clip(x, lo, hi) with lo / hi the fp32 min / max of that sample's known pixels.  Every other pixel keeps its bits.  In place.
 * status (device, n int32) per sample:
 *   >= 0  filled; the number of iterations used (0: the sample has no holes, or its right-hand side is zero and x = 0)
 *   -1    not converged within max_iter, or a breakdown (p.Ap <= 0, a non-finite scalar): the sample is left bit for bit as it was
 *   -2    every pixel is a hole: untouched            -3    more than max_unknowns holes: untouched
 * scratch: ptta_inpaint_scratch_bytes(n, height, width, max_unknowns) bytes of device memory, 16-byte aligned, contents irrelevant
 * (-22 from the size function for arguments the call would refuse, and for a size past int64).  -22 before any launch: a NULL pointer, n < 1, a size below 5,
 * height x width >= 2^31, max_unknowns < 1, max_iter < 1, an rtol that is not a positive finite number, a scratch that is too small or
 * not 16-byte aligned.  Two launches of one workgroup per sample, no atomics, no wait of one workgroup on another, every loop bounded by
 * max_iter: results are bit-identical from run to run.  Handle-free, enqueues only. */
int64_t ptta_inpaint_scratch_bytes(int n, int height, int width, int max_unknowns);
int ptta_inpaint_biharmonic(float* depth, int n, int height, int width, int max_unknowns, int max_iter, double rtol, void* scratch,
                            int64_t scratch_bytes, int32_t* status, ptta_stream s);

/* The summary panels of the plugin's log_summary (src/external_model_adapt.py:662-909) composed on device: ONE launch writes the complete
 * grid the reference hands to summary_writer.add_image -- torch.cat of the rows, torchvision's make_grid(nrow = n_image_per_summary,
 * padding 2, pad value 0) and log_utils.colorize (:53-80) included -- so that one copy of the finished grid leaves the card instead of up to
 * five fp32 maps.  Per shown sample i < n_show a panel of R rows, each `height` high and 2 `width` wide, stacked along the height, in this order:
 *   image k < n_images   left: image[k][i] after the display transform                 right: zeros
 *   PTTA_SUMMARY_ROW_OUTPUT  left: viridis(output_depth / max_predict_depth)           right: zeros
 *   PTTA_SUMMARY_ROW_SPARSE  left: viridis(sparse_depth / max_predict_depth)           right: inferno(e_s / 0.05f)
 *   PTTA_SUMMARY_ROW_GT      left: viridis(ground_truth / max_predict_depth)           right: inferno(e_g / 0.05f)
 *   e_s = validity_map > 0 ? |out - sparse| / (sparse + 1e-8f) : validity_map                       (:820-825)
 *   e_g = ground_truth > 0 ? (|out - gt| + 1e-8f) / (gt + 1e-8f) : 0                                (:846-863)
 * Display transform (:738-766): x / 255.0f when *image_div255[k] != 0 (NULL: never), then (x - rev_mean[c]) / rev_std[c] when `normalize`.
 * Colormap of x, with t = x * 256.0f in fp32: NaN -> (0, 0, 0); t < 0 -> entry 0; t >= 256 -> entry 255; else entry trunc(t); the value
 * written is the fp64 table entry rounded to fp32.  `viridis` / `inferno` are 256 x 3 fp64 device tables (matplotlib's `.colors`); the
 * library embeds none.  Every value is a table entry or a chain of single correctly rounded fp32 operations (IEEE division, no fma):
 * the grid equals the reference's bit for bit.
 * Grid: n_show == 1: the panel itself, 3 x (R height) x (2 width).  n_show > 1: 3 x (R height + 4) x (n_show (2 width + 2) + 2), panel i at
 * row 2, column i (2 width + 2) + 2, zeros elsewhere.  ptta_summary_grid_shape (pure host) returns the two sizes.
 * out: PTTA_SUMMARY_OUT_F32_CHW: fp32 3 x GH x GW.  PTTA_SUMMARY_OUT_U8_HWC: uint8 GH x GW x 3 holding (uint8) clamp(v * 255.0f, 0, 255)
 * by truncation, NaN -> 0: the conversion torch.utils.tensorboard applies to a float image.  Every output element is written exactly once
 * (padding and zero halves included): the buffer needs no clearing.  16-byte stores where the output base is 16-byte aligned and GH GW is
 * a multiple of 4 (uint8: 12 bytes per lane on a 4-byte-aligned base); one pixel per lane otherwise, same results.
 * Inputs are fp32, device, image N x 3 x height x width and the maps N x 1 x height x width with N >= n_show; only the first n_show samples are read.
 * -22 before any launch: a NULL args / output, no row at all, n_images outside 0..PTTA_SUMMARY_MAX_IMAGES, a NULL image, a row bit without
 * its inputs (OUTPUT: output_depth; SPARSE: OUTPUT + sparse_depth + validity_map; GT: OUTPUT + ground_truth), unknown row bits or out_dtype,
 * n_show < 1, a size < 1, GH GW 3 >= 2^31, a max_predict_depth that is not a positive finite number, a NULL table while a coloured
 * row is requested.  Handle-free, enqueues only, no atomics.
 *
 * ptta_summary_image_flag: the `torch.max(img) > 10.0` test of the display transform, on device: flag[0] = 1 when some element of
 * image[0 .. count) is > 10 and none is NaN (torch.max propagates NaN and NaN > 10 is false), else 0.  count covers the WHOLE tensor, not
 * only the shown samples.  `flag` is PTTA_SUMMARY_FLAG_WORDS int32 of device memory (word 0 the flag, the rest per-block partial results;
 * contents irrelevant on entry).  Two launches (per-block partials, then their union): no atomics, bit-identical from run to run, no host
 * synchronisation; pass `flag` as image_div255[k] of a compose call enqueued behind it on the same stream.  -22: a NULL or misaligned
 * pointer, count < 1. */
#define PTTA_SUMMARY_MAX_IMAGES 8
#define PTTA_SUMMARY_ROW_OUTPUT 1
#define PTTA_SUMMARY_ROW_SPARSE 2
#define PTTA_SUMMARY_ROW_GT 4
#define PTTA_SUMMARY_OUT_F32_CHW 0
#define PTTA_SUMMARY_OUT_U8_HWC 1
#define PTTA_SUMMARY_FLAG_WORDS 257
typedef struct ptta_summary_args {
    int n_show, height, width;
    int n_images;                        /* image rows, in list order */
    int rows;                            /* PTTA_SUMMARY_ROW_* bits: the depth rows behind the image rows */
    int normalize;                       /* apply (x - rev_mean[c]) / rev_std[c] to the image rows */
    int out_dtype;                       /* PTTA_SUMMARY_OUT_* */
    float max_predict_depth;
    float rev_mean[3], rev_std[3];       /* float32(-m_c / s_c), float32(1 / s_c) */
    const float* image[PTTA_SUMMARY_MAX_IMAGES];
    const int32_t* image_div255[PTTA_SUMMARY_MAX_IMAGES];
    const float* output_depth;
    const float* sparse_depth;
    const float* validity_map;
    const float* ground_truth;
    const double* viridis;
    const double* inferno;
    void* out;
} ptta_summary_args;
int ptta_summary_grid_shape(int n_show, int height, int width, int n_rows, int64_t* grid_height_host, int64_t* grid_width_host);
int ptta_summary_image_flag(const float* image, int64_t count, int32_t* flag, ptta_stream s);
int ptta_summary_compose(const ptta_summary_args* a, ptta_stream s);

/* Scoring a run on device: the tail of the reference's drivers that turns a run into the four numbers of results.txt (adaptation loop
 * src/tta_main.py:755-809, validate :975-1030), accumulated in device memory with no host synchronisation per frame.  One accumulate call
 * scores one batch of N x 1 x height x width fp32 maps inside the window [win_y : win_y + win_height, win_x : win_x + win_width] of every
 * sample (the drivers' bottom-centre crop; the whole frame is win 0, 0, height, width); nothing outside the window is read and the maps
 * need no cropped copy.
 *   mask   PTTA_SCORE_RULE_ADAPT (:776-781)       gt > 0 && !(gt < min) && !(gt > max)     a pixel equal to a bound counts
 *          PTTA_SCORE_RULE_VALIDATE (:1008-1015)  gt > 0 && gt > min && gt < max           a pixel equal to a bound does not
 *   pixel  d = 1000 gt - 1000 out;  i = 1 / (0.001 gt + 1e-9) - 1 / (0.001 out + 1e-9);  d d and i i: every product, sum and quotient a single
 *          correctly rounded fp32 operation (no fma), as the reference's fp32 tensors compute them
 *   sums   count, sum |d|, sum d d, sum |i|, sum i i in fp64, per sample and pooled over the batch
 *   batch  MAE = sum |d| / count, RMSE = sqrt(sum d d / count) in mm, iMAE, iRMSE likewise in 1/km, in fp64 from the POOLED sums (the
 *          reference takes one mean over the whole batch and multiplies it by batch_size); count == 0 gives 0 / 0 = NaN as torch.mean of
 *          an empty tensor does
 *   state  sum[k] += metric_k n (fp64);  frames += n;  batches += 1;  pixels += count;  empty_batches += (count == 0).  A NaN stays in the
 *          run; empty_batches says why.
 * state: ptta_score_state_bytes(max_n) bytes of device memory, 16-byte aligned, handed to ptta_score_reset before its first use (reset
 * zeroes the run and makes the state's size known to the later calls; a state that was never reset is refused).  Its layout, for callers
 * that read it on device:
 *   byte 0    double sum[4]                                        the run's MAE, RMSE, iMAE, iRMSE sums
 *   byte 32   int64 frames, batches, empty_batches, pixels
 *   byte 64   double last[5]: count, sum |d|, sum d d, sum |i|, sum i i     pooled, of the latest accumulate call
 *   byte 128  double sample[max_n][6]: the same five per sample of the latest call, one pad
 *   then      the per-block partial sums of the latest call
 * Optional outputs (device, NULL = not wanted): batch_out 4 fp32, the batch's four metrics; sample_out n x 4 fp32, the same from each
 * sample's own sums (NaN for a sample without a masked pixel); sample_count_out n int32.  The fp32 values are the fp64 ones rounded once.
 * ptta_score_result writes 8 doubles to device memory: MAE, RMSE, iMAE, iRMSE = sum[k] / (n_sample > 0 ? n_sample : frames) (:806-809; the
 * reference's / 1000 ... * 1000 cancels), then frames, batches, empty_batches, pixels.
 * Two launches per accumulate call: partial sums over n x B workgroups, B a fixed function of the window's size (never of timing), then
 * one workgroup that adds them in a fixed order.  No floating-point atomics, no workgroup waits on another, every loop is bounded by the
 * arguments: results are bit-identical from run to run.  Both maps are read with 16-byte loads where width, win_x and win_width are
 * multiples of 4 and both base pointers are 16-byte aligned, one pixel per load otherwise; the two paths add in different orders and may
 * differ in the last bits of the fp64 sums.  Nothing is written except the state and the optional outputs.
 * -22 before any launch, with the reason in ptta_last_error(NULL): a NULL args, map or state pointer; n < 1 or n > the state's max_n; a
 * size < 1; a window that is empty or leaves the sample; min > max or a bound that is not finite; a rule other than the two; a state that is
 * not 16-byte aligned, was not reset, or is too small (reset: state_bytes below the size for max_n = 1; the size function: max_n < 1 or
 * above PTTA_SCORE_MAX_N).  Handle-free, enqueue only; one state is used from one stream at a time. */
#define PTTA_SCORE_MAX_N 4096
enum { PTTA_SCORE_RULE_ADAPT = 0, PTTA_SCORE_RULE_VALIDATE = 1 };
typedef struct ptta_score_args {
    const float* depth;          /* N x 1 x H x W fp32, contiguous */
    const float* ground_truth;   /* same shape */
    int n, height, width;
    int win_y, win_x, win_height, win_width;   /* scoring window inside every sample */
    float min_evaluate_depth, max_evaluate_depth;
    int rule;
    void* state;                 /* ptta_score_state_bytes(max_n) bytes, 16-byte aligned */
    float* batch_out;            /* optional, 4: this batch's pooled MAE, RMSE (mm), iMAE, iRMSE (1/km) */
    float* sample_out;           /* optional, n x 4: the same per sample */
    int32_t* sample_count_out;   /* optional, n: masked pixels per sample */
} ptta_score_args;
int64_t ptta_score_state_bytes(int max_n);
int ptta_score_reset(void* state, int64_t state_bytes, ptta_stream s);
int ptta_score_accumulate(const ptta_score_args* a, ptta_stream s);
int ptta_score_result(const void* state, int64_t n_sample, double* out8, ptta_stream s);   /* out8 on the device */

/* The other augmentations the adapt scripts enable (bash/adapt/adapt_msgchn_vkitti.sh:34-41; applied in every step,
 * src/tta_main.py:595-605).  The reference implements them with torchvision.transforms.functional 0.10.1 (third party, absent
 * from the reference tree: parity unpinned); each call restates torchvision's tensor algorithm.  All handle-free, enqueue only,
 * per-sample decisions as device arrays (uint8 flags; a sample whose flag is 0 is copied), dst must not alias src.
 *   ptta_rotate         Transforms.rotate (src/transforms.py:1036-1070): functional.rotate(image, angle[b] degrees, interpolation,
 *                       expand=False): affine grid about the image centre + grid_sample(align_corners=False, zeros);
 *                       bilinear = 0 nearest (depth, validity, ground truth), 1 bilinear (image)  (src/tta_main.py:471-473)
 *   ptta_resize_crop    Transforms.resize_and_crop (:1222-1283): functional.resize to (resize_height[b], resize_width[b]) then the crop
 *                       [start_y[b] : +height, start_x[b] : +width] back to the input size; scale_depth = resize_scaling_depth
 *   ptta_photometric    brightness -> contrast -> saturation (:714-838, :236-311) on uint8-valued 3-channel images (the reference casts
 *                       float images to uint8 first); any do_* pointer may be NULL (transform not configured); scratch: 256*n doubles */
int ptta_rotate(const float* src, float* dst, int n, int channels, int height, int width, const uint8_t* do_rotate, const float* angle_deg,
                int bilinear, ptta_stream s);
int ptta_resize_crop(const float* src, float* dst, int n, int channels, int height, int width, const uint8_t* do_resize,
                     const int32_t* resize_height, const int32_t* resize_width, const int32_t* start_y, const int32_t* start_x,
                     int bilinear, int scale_depth, ptta_stream s);
int ptta_photometric(const float* src, float* dst, int n, int height, int width, const uint8_t* do_brightness, const float* f_brightness,
                     const uint8_t* do_contrast, const float* f_contrast, const uint8_t* do_saturation, const float* f_saturation,
                     double* scratch, ptta_stream s);

/* The augmentations of Transforms that NO adapt script enables (src/transforms.py:279-305 gamma / hue, :322-332 noise, :508-625 crop-and-pad /
 * resize-and-pad, :630-655 patch removal).  gamma / hue / pad / resize are torchvision 0.10.1 calls in the reference (parity unpinned,
 * restated); add_noise, remove_random_patches and the crop / pad index arithmetic are the reference's own torch code (pinned:
 * tests/golden/transforms_extra.npz).  Handle-free, enqueue only, per-sample decisions as device arrays, dst must not alias src.
 *   ptta_photometric_full  brightness -> contrast -> gamma -> hue -> saturation (:236-311).  uint8 path when brightness / contrast / hue /
 *                          saturation is configured (non-NULL do_*; :102-106); with gamma alone the images stay float and torchvision's
 *                          float branch applies: (x ** gamma).clamp(0, 1).  scratch: 256*n doubles (not needed for gamma alone)
 *   ptta_add_noise         Transforms.add_noise (:839-876): dst = src + spread * noise (uniform = 0) or src + spread * (noise - 0.5)
 *                          (uniform = 1) where do_noise[b]; `noise` = the caller's torch.randn / torch.rand field, same shape as src
 *   ptta_remove_patches    Transforms.remove_random_patches (:878-924) behind random_nonzero's selection (:926-953): selected = n x H x W
 *                          bytes, 1 at the chosen nonzero pixels; every pixel within the (patch_height[b], patch_width[b]) patch of a
 *                          chosen pixel is zeroed in all channels
 *   ptta_crop_pad          Transforms.crop_and_pad (:1072-1135): image[start_y:end_y, start_x:end_x] padded by pad_top / pad_left (and what
 *                          remains below / right) back to height x width; padding_mode 0 constant (fill), 1 edge, 2 reflect, 3 symmetric
 *   ptta_resize_pad        Transforms.resize_and_pad (:1137-1220): functional.resize to (resize_height[b], resize_width[b]) <= (height,
 *                          width), then padded back to height x width as ptta_crop_pad */
int ptta_photometric_full(const float* src, float* dst, int n, int height, int width, const uint8_t* do_brightness, const float* f_brightness,
                          const uint8_t* do_contrast, const float* f_contrast, const uint8_t* do_gamma, const float* f_gamma,
                          const uint8_t* do_hue, const float* f_hue, const uint8_t* do_saturation, const float* f_saturation,
                          double* scratch, ptta_stream s);
int ptta_add_noise(const float* src, const float* noise, float* dst, int n, int channels, int height, int width, const uint8_t* do_noise,
                   float spread, int uniform, ptta_stream s);
int ptta_remove_patches(const float* src, float* dst, int n, int channels, int height, int width, const uint8_t* do_remove,
                        const uint8_t* selected, const int32_t* patch_height, const int32_t* patch_width, ptta_stream s);
int ptta_crop_pad(const float* src, float* dst, int n, int channels, int height, int width, const uint8_t* do_crop_pad,
                  const int32_t* start_y, const int32_t* start_x, const int32_t* end_y, const int32_t* end_x,
                  const int32_t* pad_top, const int32_t* pad_left, int padding_mode, float fill, ptta_stream s);
int ptta_resize_pad(const float* src, float* dst, int n, int channels, int height, int width, const uint8_t* do_resize_pad,
                    const int32_t* resize_height, const int32_t* resize_width, const int32_t* pad_top, const int32_t* pad_left,
                    int bilinear, int padding_mode, float fill, ptta_stream s);

/* The augmented inner loop's frame set through ONE draw in one launch (src/tta_main.py:595-604: the geometric transform of [image, sparse
 * depth, validity map, ground truth], then the photometric transform of the transformed image), for the draws the adapt scripts enable:
 * crop to shape, horizontal / vertical flip, rotation, resize-and-crop, brightness / contrast / gamma / hue / saturation.
 *   geometry   the staged chain ptta_crop_flip -> ptta_rotate -> ptta_resize_crop composed backwards from the output pixel; per sample a
 *              stage whose flag is 0 is the identity.  The three one-channel maps are sampled nearest (each stage gathers one pixel or
 *              a zero), the image nearest or bilinear (image_bilinear): resize's 4 taps, each a rotated pixel of 4 taps of the cropped /
 *              flipped source, in the staged kernels' operation order and rounding: every output equals the staged calls' bit for bit.
 *              scale_depth = resize_scaling_depth: every map, the validity map included, is divided by resize_width / crop_width.
 *   outputs    loss_image n x 3 x crop_height x crop_width and the maps' outputs n x 1 x crop_height x crop_width.  A NULL map is skipped
 *              together with its output (both NULL or neither).  image1 (optional): loss_image through ptta_photometric_full's uint8
 *              path, i.e. truncated to 0..255, then brightness in the same launch, then contrast / gamma / hue / saturation by a second
 *              launch iff `pass2` (the caller sets it when any sample's flag of those four is set; unset, the second launch is skipped
 *              and flags of those four are ignored).  With image1 NULL the photometric fields are not read.
 *   draws      n records in device memory, one per sample (52 bytes, no padding).  Per-sample values as ptta_crop_flip / ptta_rotate /
 *              ptta_resize_crop / ptta_photometric_full take them: crop start (clamped into the frame), angle in degrees as fp32,
 *              resize_height / resize_width / resize_y / resize_x, the five factors.
 *   scratch    ptta_augment_scratch_bytes(n, crop_height, crop_width) bytes, 8-byte aligned, needed with image1 only: the 256 * n doubles
 *              of partial grey sums the second launch reads, the per-block sums they are added from (the grid is one thread per output
 *              pixel, whatever the frame's size; the sums are of integers, exact in any order), the second launch's per-sample tables
 *              and one arrival counter per sample.  Zero it once before its first use; every call leaves the counters zero.
 * One thread per output pixel writes that pixel of every output; no thread forms an address outside its sample whatever the records hold
 * (every gather index is clamped into the cropped window).  Handle-free, enqueue only, one scratch per stream at a time.
 * -22 before any launch, with the reason in ptta_last_error(NULL): a NULL args, image, loss_image or draws pointer; a map without its
 * output or an output without its map; buffers that overlap; n outside 1..65535; a size < 1 or a frame of 2^31 values or more; a crop
 * larger than the frame; image1 without a scratch of that size and alignment. */
enum { PTTA_AUG_HFLIP = 1, PTTA_AUG_VFLIP = 2, PTTA_AUG_ROTATE = 4, PTTA_AUG_RESIZE = 8, PTTA_AUG_BRIGHTNESS = 16, PTTA_AUG_CONTRAST = 32,
       PTTA_AUG_GAMMA = 64, PTTA_AUG_HUE = 128, PTTA_AUG_SATURATION = 256 };
typedef struct ptta_augment_draw {
    uint32_t flags;                       /* PTTA_AUG_*: this sample's coins */
    int32_t crop_y, crop_x;               /* crop start (0, 0 with crop_height == height, crop_width == width: no crop) */
    float angle_deg;
    int32_t resize_height, resize_width, resize_y, resize_x;
    float brightness, contrast, gamma, hue, saturation;
} ptta_augment_draw;
typedef struct ptta_augment_args {
    const float* image;                   /* n x 3 x height x width fp32, contiguous */
    const float* sparse_depth;            /* n x 1 x height x width, or NULL */
    const float* validity_map;            /* likewise */
    const float* ground_truth;            /* likewise */
    float* loss_image;                    /* n x 3 x crop_height x crop_width */
    float* sparse_depth_out;              /* n x 1 x crop_height x crop_width; NULL iff its input is */
    float* validity_map_out;
    float* ground_truth_out;
    float* image1;                        /* n x 3 x crop_height x crop_width, or NULL */
    const ptta_augment_draw* draws;       /* n records, device memory */
    int n, height, width, crop_height, crop_width;
    int image_bilinear, scale_depth, pass2;
    void* scratch; int64_t scratch_bytes;
} ptta_augment_args;
int64_t ptta_augment_scratch_bytes(int n, int crop_height, int crop_width);
int ptta_augment_frames(const ptta_augment_args* a, ptta_stream s);

/* ptta_step enqueues its kernels directly; with ptta_set_option(h, "graph", 1) it replays a captured hipGraph of the whole step.  Graphs are re-captured after any re-binding. */
/* model.convert_syncbn() (src/tta_main.py:326 -> SyncBatchNorm.convert_sync_batchnorm, src/msg_chn_model_adapt.py:547-556)
 * for the one-process-per-GPU run with shared adapted parameters: every training-mode BatchNorm then normalises with
 * the statistics of the GLOBAL batch.  The library collapses a BatchNorm's partial sums into `exchange_buf` (device,
 * float64, caller-owned, `capacity` elements >= 2 * 2 * widest BatchNorm), calls `fn(user, exchange_buf, count, stream)`
 * -- which must SUM the first `count` elements over the ranks in place, ordered on `stream` (torch.distributed.all_reduce
 * on RCCL does exactly that) -- and finalises with world_size x the local row count (equal local batches).  Gradients of
 * adapted BatchNorm parameters come out already averaged over the ranks.  world_size 1 switches the exchange off (and
 * restores graph replay / the second stream).  MSG_CHN handles replay no hipGraph while the CALLBACK form is on. */
typedef int (*ptta_allreduce_fn)(void* user, double* exchange_buf, long long count, ptta_stream s);
int ptta_set_stat_sync(ptta_handle h, ptta_allreduce_fn fn, void* user, double* exchange_buf, int64_t capacity, int world_size);

/* The same exchange on an RCCL communicator owned by the library (the reference's backend: dist.init_process_group('nccl'),
 * src/tta_main.py:101-111): rank 0 calls ptta_rccl_unique_id, the caller broadcasts the 128 bytes, every rank calls
 * ptta_rccl_comm_create (ncclCommInitRank) and ptta_set_stat_sync_rccl.  The library enqueues ncclAllReduce itself on the
 * step's stream: no host callback, and the collectives are captured into the step's hipGraph (MSG_CHN handles keep replaying).
 * comm == NULL switches the exchange off.  ptta_rccl_allreduce_mean_f32 is the ONE gradient collective of a shared-parameter step
 * (the adapted gradients only, instead of DDP's all-reduce of every gradient: src/msg_chn_model_adapt.py:476-480).
 * librccl is resolved at run time (the process's own copy first); -38 when it cannot be loaded; ptta_rccl_last_error() for RCCL errors. */
int ptta_rccl_unique_id(void* id128_host);
int ptta_rccl_comm_create(const void* id128_host, int rank, int world_size, void** comm_out_host);
int ptta_rccl_comm_destroy(void* comm);
int ptta_rccl_allreduce_mean_f32(void* comm, float* buf, int64_t count, ptta_stream s);
const char* ptta_rccl_last_error(void);
int ptta_set_stat_sync_rccl(ptta_handle h, void* comm, double* exchange_buf, int64_t capacity, int world_size);
/* DistributedDataParallel's gradient averaging inside the fused ptta_step (src/tta_main.py:354,631-633): between backward and
 * Adam the adapted gradients are averaged over the communicator with one ncclAllReduce on the step's stream.  NULL: off. */
int ptta_set_grad_sync_rccl(ptta_handle h, void* comm);

int ptta_set_graph(ptta_handle h, int enable);         /* = ptta_set_option(h, "graph", enable) */

/* Per-handle switches -- the library's ONLY run-time configuration besides the ptta_hparams struct: no environment variable is read after
 * ptta_create (the three create-time validation variables are listed at the end of this comment).  Setting an option waits for the
 * handle's streams and drops its captured graphs; the next step re-captures.  Every non-default value is a correct, slower form of
 * the same step, kept as the check of the default (tests/test_gpu_options.py) or taken by the library itself where the default
 * form does not apply (small maps, N > 16, SyncBatchNorm exchange).  Unknown key / value out of range: -22; a key the handle does
 * not have: -38 (the generic engine has "graph", "head_bn_fused", on NLSPN handles that train "deterministic" and, on PTTA_ADAPT_META_ONLY handles, "eval_bn_fused"; PTTA_DTYPE_MIXED handles keep every key but graph / aux_stream / thru / adam_in_wgrad / pair_fuse / tpair_fuse at 1).
 *   key             default  meaning of 0
 *   "graph"         0        (1:) ptta_step / ptta_step_pipelined / ptta_forward_eval replay captured hipGraphs from their second call on.  Default
 *                            since round 5: direct launches on the caller's stream and the handle's own streams -- measured FASTER than replay
 *                            on ROCm 7.2 for all three engines (MSG_CHN pipelined 1.28 vs 1.31 ms, call by call 1.45 vs 1.52: a replayed
 *                            graph starts its second branch late and runs it slower, profiles/r05_step_stamps.txt; host cost 0.46 ms per call)
 *   "aux_stream"    1        one stream: no second queue for the proxy chain / the heads
 *   "thru"          1        the heads' stream joins the main stream before the loss (1: it runs on into loss + head backward)
 *   "adam_in_wgrad" 1        0: Adam is its own launch behind the weight gradient's reduction (1: that reduction applies it -- MSG_CHN 1layer, no
 *                            gradient exchange between the two; one dependent launch less at the end of the step)
 *   "bwd_w2"        1        (PTTA_DTYPE_MIXED) 0: the narrow data-gradient convolutions take bf16-ROUNDED weights, one MFMA per product (round 5's
 *                            form); 1: weights as bf16 hi + lo, two MFMAs per product, gradient maps still bf16 in HBM.  A rounded weight is a
 *                            systematic 2^-9 error of the gradient's direction, the same at every pixel and step: over 150 steps at 256x320 it
 *                            put the scored depth at 1.1e-3 from the reference (3x the reference's own 1-ulp sensitivity); with hi + lo
 *                            weights the mixed mode stays at that floor (profiles/r06_drift.txt).  Not bit-identical to 0 by construction
 *   "fuse_first"    1        every first-layer convolution + the following 32->32 convolution as two launches (2: the RGB branch fused too)
 *   "fuse_head_bwd" 1        the prediction heads' backward as separate launches
 *   "fuse_heads"    1        proj -> pred as separate Linear launches (1: pred.0 o proj.3 folded into one weight at load time)
 *   "heads_v2"      1        proj's hidden layer materialised (1: recomputed inside the GEMM from analytic BatchNorm statistics)
 *   "cos_in_gemm"   1        d loss_cos / d ref written as a tensor (1: formed in the backward GEMM's operand staging)
 *   "mask_bits"     1        fp32 pre-activation maps as ReLU masks (1: one word of sign bits per pixel)
 *   "pair_fuse"     1        every (stride-2 -> stride-1) layer pair as two launches (1: ONE launch where the stride-1 half runs on a small map --
 *                            at most 256 tiles of 8 x 32 -- and the pair is an instantiated form, csrc/conv_pair.hip: the three encoder pairs of
 *                            stages 2 and 3 at 1/4 and 1/8 resolution, fp32 and narrow maps, and on PTTA_DTYPE_MIXED handles the three
 *                            stride-2 pairs of the data gradients).  Bit-identical (tests/test_gpu_conv_pair.py);
 *                            free on PTTA_DTYPE_MIXED handles
 *   "tpair_fuse"    1        every (transposed -> stride-1) layer pair as two launches (1: ONE launch where the pair is an instantiated form,
 *                            csrc/conv_tpair.hip, at every map size in the forward: the two decoder pairs of stage 2 on both chains and the two of
 *                            decoder 3, fp32 and narrow maps; persistent 8 x 32 tiles where the stride-1 half would take them, 4 x 32 tiles on
 *                            small maps.  The intermediate 32-channel map is then not written where nothing but the stride-1 layer reads its
 *                            values -- always, unless the backward masks with the float map ("mask_bits" 0) -- and ptta_debug_tensor refuses
 *                            "t2", "u2", "t3", "u3" with -38 while that holds.  On PTTA_DTYPE_MIXED handles also the data gradients' four
 *                            transposed pairs of encoders 3 and 2, where a launch has at most one tile per block (480 tiles of 8 x 32: at
 *                            352 x 1216, batch 1, the 1/4- and 1/2-resolution pairs; the full-resolution pair measured slower as one launch
 *                            and stays two).  Bit-identical (tests/test_gpu_conv_tpair.py); free on PTTA_DTYPE_MIXED handles
 *   "stamps"        0        (diagnostic, 1:) fourteen one-thread nodes of the step's and the prefix's graphs write wall_clock64() ticks since
 *                            the step's first node into the debug tensor "stamps" -- where the branches of a replayed step start and end with
 *                            no profiler attached (tools/step_stamps.py, profiles/r05_step_stamps.txt); results unchanged
 *   "eval_bn_fused" 1        (PTTA_ADAPT_META_ONLY handles only, the source model PTTA_META_NONE | PTTA_ADAPT_META_ONLY among them; -38 elsewhere) 0: every BatchNorm2d of the eval forward is its own apply launch
 *                            from the same affine table (1: in the epilogue of the convolution in front of it).  Bit-identical
 *                            (tests/test_gpu_nlspn_meta.py): both forms compute fmaf(conv + bias, scale, shift).  On CostDCNet's source model
 *                            (PTTA_COSTDC_PLAIN | PTTA_ADAPT_META_ONLY) the switch covers the 28 BatchNorm3d + ELU as well
 *                            (tests/test_gpu_costdc_source.py)
 *   "head_bn_fused" 1        (NLSPN and CostDCNet handles; -38 on MSG_CHN, which has no BatchNorm2d) 0: in the stage-2 head trainer's two
 *                            no-gradient backbone passes (ptta_head_forward / ptta_head_step, both forms of ptta_head_set_form) every frozen
 *                            BatchNorm2d is an affine-table launch and an apply launch of its own (1: all tables of the prefix are built by ONE
 *                            launch per head forward, from the gamma / beta bound at that call, and each BatchNorm2d runs in the epilogue of the
 *                            convolution in front of it: NLSPN's conv1 .. conv6, CostDCNet's Encoder2D, the 2layers block of either; bf16x6
 *                            images keep bf16x6).  Bit-identical (tests/test_gpu_head_bn_fused.py).  BatchNorm3d, the sparse encoder's
 *                            BatchNorm, the heads' BatchNorm1d and PTTA_DTYPE_MIXED handles keep their separate launches either way.  With 1 a
 *                            head forward does not write the raw convolution outputs of the fused pairs (see ptta_debug_tensor).
 *                            Measured on MI355X, head step, 1 against 0 alternating in one process (profiles/head_bn_fused.txt,
 *                            tools/bench_head_generic.py): NLSPN 352x1216 9.49 against 10.63 ms (N 1), 17.47 against 19.66 (N 2); CostDCNet 480x640
 *                            4.94 against 5.42 (N 1), 8.31 against 9.21 (N 2); 0 equals the step before the option within the run-to-run spread.
 *                            Faster on both backbones, hence 1 on both
 *   "deterministic" 0        (NLSPN handles with a backward: 1layer, 2layers, PTTA_ADAPT_META_ONLY, PTTA_META_NONE, PTTA_NLSPN_SYNCBN_ADAPT, both dtypes;
 *                            -38 with a reason on MSG_CHN and CostDCNet, whose steps are bit-reproducible as they are,
 *                            and on the source model PTTA_META_NONE | PTTA_ADAPT_META_ONLY, which has no backward)  0: the 18 propagation
 *                            sweeps' feature gradient and the affinity gradient's confidence gradient are scattered with float atomicAdd (LDS +
 *                            global): the order the atomics arrive in decides the rounding, two runs of one build differ by ~5e-6 relative in the
 *                            gradients.  1: the same two scatters add 64-bit FIXED-POINT integers instead (ds_add_u64 on the LDS tile, 64-bit
 *                            global atomics), llrintf(contribution * 2^S), and a convert launch per scatter turns the int64 map into fp32.
 *                            Integer addition is associative: the same frames give the same bits on every run, direct launches or graph replay.
 *                            S is chosen on the device, per launch, so that overflow is impossible: 2^S * (bound of the sum of |contributions|)
 *                            <= 2^60, the bound being N*H*W * max|gout| * max_pixel(sum_k |affinity_k|) for a sweep and 8 * N*H*W * max|g_c| for
 *                            the confidence gradient, each maximum reduced on the device with integer atomicMax on the fp32 bit patterns (no host
 *                            read: the step stays capturable) and rounded up to a power of two.  Quantum: 2^-S, at most 2^-57 of that bound
 *                            (N*H*W = 2^20, affinities summing to 3: below 2^-34 of max|gout|).  Per element: every contribution is rounded by
 *                            at most half a quantum, then the sum is rounded ONCE to fp32 -- |error| <= K * 2^-S / 2 + 2^-24 |sum| for K
 *                            contributions, where the float form rounds by up to 2^-24 of the running sum at each of its K additions in an
 *                            arbitrary order.  A maximum of 0 gives a zero map; a non-finite maximum (inf or NaN anywhere in gout, the
 *                            affinities or g_c) gives a map of NaN in every element, where the float form spreads it sweep by sweep.  The gathers
 *                            (offset and tap-affinity gradients, the g_oa channels) keep their arithmetic bit for bit
 *                            (tests/test_gpu_nlspn_det_elementwise.py).  Memory: 8 bytes per pixel of the batch + 256 bytes, allocated when the
 *                            option is first set to 1.  Not bit-identical to 0 by construction; same error class (the tests hold 1 to twice the
 *                            measured error of 0 against an fp64 reference).  Measured on MI355X, 352x1216, 1 against 0 alternating in one
 *                            process (profiles/nlspn_deterministic.txt, tools/bench_nlspn_deterministic.py): 21.75 against 20.26 ms per step
 *                            (N 1, fp32), 20.98 against 19.54 (N 1, mixed), 40.68 against 37.43 (N 2, fp32), 39.06 against 35.92 (N 2, mixed);
 *                            one sweep's gradient 140 against 74 us (the 64-bit LDS atomic runs at about half the rate of the float one);
 *                            0 equals the step before the option within the run-to-run spread.  Slower, hence 0
 * Read-only keys (ptta_get_option; -22 from ptta_set_option):
 *   "pipelined_active"  1 when ptta_step_pipelined runs as itself on this handle as configured now; 0 when it degrades to ptta_step call by call
 *                       (generic-engine backbones, the dual-corner padded path, a statistics exchange or a gradient communicator bound,
 *                       validation arithmetic, the profiling leg) -- same results, the call-by-call price
 *   "thru_active"       1 when the step takes the two-stream `thru` schedule
 *   "head_bn_fused_count"  how many BatchNorm2d of this handle's stage-2 prefix ride in a convolution epilogue as configured now: 36 (NLSPN),
 *                       38 (NLSPN 2layers), 15 (CostDCNet), 17 (CostDCNet 2layers); 0 with "head_bn_fused" 0, on a PTTA_DTYPE_MIXED handle and with
 *                       PTTA_CONV_IMPL=naive (no matrix-core convolution to ride in); -38 on MSG_CHN
 *   "eval_bn_fused_count"  (PTTA_ADAPT_META_ONLY handles; -38 elsewhere) how many BatchNorm of the eval forward ride in a convolution epilogue as
 *                       configured now: 43 on CostDCNet's source model (15 BatchNorm2d + 28 BatchNorm3d); 0 with "eval_bn_fused" 0
 *   "pair_fuse_count"   how many layer pairs the last step issued as one launch ("pair_fuse"; a replayed graph: as it was captured); 0 with
 *                       "pair_fuse" 0, on maps too large for the form, with PTTA_CONV_IMPL=naive and PTTA_ARITH=exact
 *   "tpair_fuse_count"  the same count for "tpair_fuse"; 0 with "tpair_fuse" 0, with PTTA_CONV_IMPL=naive and PTTA_ARITH=exact
 * bit-identical to the default: aux_stream, thru, adam_in_wgrad, fuse_first, fuse_head_bwd, mask_bits, graph, pair_fuse, tpair_fuse; within bf16x3's own error (documented
 * in the tests): fuse_heads, heads_v2, cos_in_gemm.
 * Environment, read once per ptta_create (csrc/ptta_kernels.h ptta_create_env) because it decides allocation and arithmetic:
 *   PTTA_CONV_IMPL=naive (direct fp32 kernels, PTTA_DTYPE_F32 only), PTTA_ARITH=exact (fp32 MFMA, MSG_CHN PTTA_DTYPE_F32 only),
 *   PTTA_GRAPH=0|1 (initial value of "graph").  Recommended for the hosting process, not set by the library: HIP_FORCE_DEV_KERNARG=1
 *   before the HIP runtime initialises (kernel arguments in device memory: -7 % on the replayed step). */
int ptta_set_option(ptta_handle h, const char* key, int value);
int ptta_get_option(ptta_handle h, const char* key, int* value_host);

/* Measurement hook for bench.py: while enabled, the step runs kernel by kernel on one stream and EVERY launch is bracketed by hipEvents
 * on that stream, accounted to one of nine classes:  0 / 1 stride-1 3x3 32->32 convolution with ReLU on load, maps above / up to 1/4
 * resolution (together: the dominant kernel class of bench.py's `roofline`);  2 / 3 the same without ReLU (data gradients);  4 / 5 stride-2
 * and transposed convolutions;  6 the MLP heads (GEMMs + BatchNorm finalize);  7 first-layer / prediction convolutions (Cin <= 3 or
 * Cout = 1) and their data gradients;  8 everything else (resampling, loss, weight gradient, Adam, packing).  read returns the summed
 * duration (ms), the algorithmic bytes and MACs (SURVEY.md 8d counting rule: input + output + weight elements per conv / linear layer,
 * 0 for class 8) and the launch count since enable, after synchronising s. */
int ptta_profile(ptta_handle h, int enable);
int ptta_profile_read(ptta_handle h, int klass, double* ms_total_host, double* alg_bytes_host, double* macs_host,
                      int64_t* launches_host, ptta_stream s);

/* Test / debug hooks (not on the hot path).  ptta_debug_tensor reads a named activation of the last forward.  With "head_bn_fused" 1 a head
 * forward does NOT write the raw convolution output in front of a fused BatchNorm2d (NLSPN "conv2.0.r1", CostDCNet "enc2d.layer1.0.r1", ...;
 * likewise "eval_bn_fused" and the eval forward of a PTTA_ADAPT_META_ONLY handle): such a name then returns what an earlier TTA forward left
 * there.  Set the option to 0 to read them.  With "tpair_fuse" 1 the MSG_CHN forward does not write the intermediate maps "t2", "u2", "t3", "u3" of its
 * fused (transposed -> stride-1) pairs: reading one of them then FAILS with -38 instead of returning an earlier step's values; set "tpair_fuse" 0. */
int ptta_debug_tensor(ptta_handle h, const char* name, float* dst, int64_t capacity, int64_t* numel_host, ptta_stream s);
int ptta_op_conv32(const float* in_nhwc, const float* weight, const float* bias, float* out_nhwc,
                   int b, int hin, int win, int mode, int relu_in, int in_major, int flip, int dtype, int naive,
                   ptta_stream s);
/* Test hook: a (stride-2 | transposed, first_mode 1 | 2) 32->32 convolution followed by a stride-1 one, fp32 NHWC device buffers, as the MSG_CHN
 * engine issues such a pair: relu1 / relu2 = ReLU on the first / second layer's input; the first layer's ReLU mask as one word of sign bits
 * per pixel (mask1_bits [b][hm][wm]) and its addend add0 [b][hm][wm][32] -- with add0 the second layer reads the first one's SUM; the second
 * layer's bilinear x2 skip `up` [b][hm/2][wm/2][32], skip addends add1, add2 (their sum goes to out_sum) and mask words mask2_bits (each
 * may be NULL); in_nb <= b frames of input (frame b % in_nb); dtype PTTA_DTYPE_F32 (bf16x3) or any other (narrow maps); w2 = the hi + lo
 * weight form of the narrow data gradients.  fused 1: ONE launch where the pair is an instantiated form on a small map
 * (csrc/conv_pair.hip), otherwise and with fused 0 two launches; *fused_host = 1 iff the one-launch form ran.  Outputs (NULL: not wanted):
 * the second layer's map / sum, the first layer's map, sum and (PTTA_DTYPE_F32) sign-bit words.  The two forms are bit-identical.
 * Synchronises. */
int ptta_op_conv32_pair(const float* in_nhwc, const float* weight1, const float* bias1, const float* weight2, const float* bias2,
                        const float* up_nhwc, const float* add0_nhwc, const float* add1_nhwc, const float* add2_nhwc,
                        const uint32_t* mask1_bits, const uint32_t* mask2_bits, float* out_raw, float* out_sum, float* mid_raw,
                        float* mid_sum, uint32_t* mid_bits, int b, int in_nb, int hin, int win, int first_mode, int relu1, int relu2,
                        int in_major, int flip, int dtype, int w2, int fused, int* fused_host, ptta_stream s);
/* Test hook: the same pair and operand set with the one-launch form of csrc/conv_tpair.hip (a TRANSPOSED first half, first_mode 2; any other
 * pair takes the two launches).  form 0 = as the step would choose by the map size, 1 = 4 x 32 one-tile blocks, 2 = persistent 8 x 32 tiles;
 * max_blocks > 0 caps the grid, so that a small map makes a block walk several tiles (0: no cap).  With mid_raw NULL the one-launch form does
 * not write the first layer's map (its sign-bit words still are); the hook then checks that the map's buffer still holds its fill (-14 if
 * not).  form 0 also applies the step's rule of where the one launch pays (the data gradients' form: at most 480 tiles of 8 x 32).  *fused_host = 1 iff the one-launch form ran.  form outside 0 .. 2 or
 * max_blocks < 0: -22.  Synchronises. */
int ptta_op_conv32_tpair(const float* in_nhwc, const float* weight1, const float* bias1, const float* weight2, const float* bias2,
                         const float* up_nhwc, const float* add0_nhwc, const float* add1_nhwc, const float* add2_nhwc,
                         const uint32_t* mask1_bits, const uint32_t* mask2_bits, float* out_raw, float* out_sum, float* mid_raw,
                         float* mid_sum, uint32_t* mid_bits, int b, int in_nb, int hin, int win, int first_mode, int relu1, int relu2,
                         int in_major, int flip, int dtype, int w2, int fused, int form, int max_blocks, int* fused_host, ptta_stream s);
/* Diagnostic (tests, tools/bench_gwgrad_wide.py): weight and bias gradient of a stride-1 3x3 convolution, dense fp32 NHWC device maps
 * x [b][h][w][ci] and gy [b][h][w][co], 1 <= ci, co <= 256 -> gw [co][ci][3][3], gb [co] (gb may be null).  impl 0: the launcher the engine
 * runs -- bf16x3 on the matrix cores (hi*hi + hi*lo + lo*hi, fp32 accumulation) for Ci, Co <= 64, 32 <-> 128 and, for channel counts that
 * are multiples of 16 up to 256 with more than one 32 x 32 tile pair (16 -> 64, 48 <-> 256), the wide form; the fp32-MFMA form otherwise;
 * impl 1: the fp32-MFMA form for every shape; impl 2: the direct fp32 form of PTTA_CONV_IMPL=naive.  Deterministic: fixed-order
 * reduction, no atomics.  reps > 0: `reps` more calls of the same form timed with hipEvents on s, microseconds per call (weight-gradient
 * kernel + its reduction) to *us_per_call_host; reps = 0 and us_per_call_host = NULL compute once.  Synchronises. */
int ptta_op_gwgrad(const float* x_nhwc, const float* gy_nhwc, float* gw, float* gb, int b, int h, int w, int ci, int co, int impl,
                   int reps, float* us_per_call_host, ptta_stream s);
/* Test hook: ONE convolution of the generic op-list engine (NLSPN, CostDCNet, the 2layers block) on fp32 NHWC device views, packed and
 * launched the way the engine does it.  Sources x0 [b][hin][win] (c0 channels, pixel stride ld0 >= c0) and, channel-concatenated behind
 * it, optional x1 (c1, ld1; NULL and 0 without); output view y [b][hout][wout] (co channels, pixel stride ldy; channels outside the view
 * are not touched).  weight as the state dict holds it: [co][c0 + c1][k][k], [c0 + c1][co][k][k] for PTTA_GCONV_T2, [co][ci][3][1][1]
 * with PTTA_GCONV_VERT (a 3x1x1 Conv3d run as a vertical 3-tap convolution: k = 3, stride 1); bias [co] or NULL; k 1 or 3.
 * geom: PTTA_GCONV_S1 (hout = hin), _S2 (stride 2, hout = ceil(hin / 2)), _T2 (transposed, stride 2, output_padding 1: hout = 2 hin).
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 sigmoid, applied to (accumulate ? y : 0) + bias + convolution.
 * impl 0: the matrix-core kernels (channel counts multiples of 8, of 16 for the strided geometries; 16-byte aligned sources); impl 1: the
 * direct fp32 kernels, one launch per source.  Arithmetic of impl 0, per image of the batch: images below six_b bf16x6, the others
 * bf16x3; images from x1_from_b on (pass b or more for none) one bf16 product (x_hi w_hi), with PTTA_GCONV_X1_W2 two (x_hi (w_hi + w_lo)).
 * PTTA_GCONV_DGRAD: the data gradient instead, as the engine's backward sweep runs it: x0 = the gradient of the forward OUTPUT
 * ([b][hin][win][c0], c0 = the forward convolution's output channels, no x1), weight = the FORWARD weight of a co -> c0 convolution of
 * geometry geom, y = the gradient of its input (S2: hout = 2 hin or 2 hin - 1; T2: hout = hin / 2).
 * stat_npass 1 or 2 (S1, impl 0): the fused BatchNorm partial sums of the epilogue, summed over the tiles, to stat_host [npass][2][co] =
 * {sum y, sum y^2} per equal slice of the batch; 0 and NULL without.  form_host (may be NULL): for the strided geometries of impl 0 the
 * kernel form the launcher took -- 0: one channel tile per wave, 1: two, 2: K split over the block's waves -- else -1.
 * -22 for arguments outside this, -12 out of memory.  Synchronises. */
#define PTTA_GCONV_S1 0
#define PTTA_GCONV_S2 1
#define PTTA_GCONV_T2 2
#define PTTA_GCONV_VERT 1
#define PTTA_GCONV_X1_W2 2
#define PTTA_GCONV_DGRAD 4
#define PTTA_GCONV_AFF_ACT_FIRST 8      /* ptta_op_gconv_affine only (-22 from ptta_op_gconv) */
#define PTTA_GCONV_AFF_RES_PLAIN 16     /* ptta_op_gconv_affine only */
int ptta_op_gconv(const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, const float* weight, const float* bias, float* y,
                  int co, int ldy, int b, int hin, int win, int hout, int wout, int k, int geom, int act, int accumulate, int impl,
                  int flags, int six_b, int x1_from_b, int stat_npass, double* stat_host, int* form_host, ptta_stream s);
/* The same hook with the epilogue of the PTTA_ADAPT_META_ONLY eval forward and of the stage-2 head trainer (option "head_bn_fused"): a
 * BatchNorm2d with constant statistics behind the convolution,
 *   y = act(fmaf(conv + bias, scale[c], shift[c]) [+ res])                    no flag; with res: act 1, the BasicBlock's ReLU behind the sum
 *   y = relu(relu(fmaf(conv + bias, scale[c], shift[c])) + res)               PTTA_GCONV_AFF_ACT_FIRST: CostDCNet's ResBlock; res and act 1 required
 *   y = fmaf(conv + bias, scale[c], shift[c]) + res                           PTTA_GCONV_AFF_RES_PLAIN: the 2layers block's last BatchNorm2d; res and act 0
 *   v = fmaf(conv + bias, scale[c], shift[c]); y = v > 0 ? v : expm1f(v)      act 4 (ELU), no flag or PTTA_GCONV_VERT: CostDCNet's BatchNorm3d + ELU behind
 *                                                                             its 1x3x3 / 3x1x1 convolution (the source model's eval forward); PTTA_GCONV_S1,
 *                                                                             k = 3, no res; bf16x3 and, below six_b, bf16x6 (tests/test_gpu_gconv_affine_elu.py)
 * scale / shift [co]: the {scale, shift} rows of an eval affine table (what PTTA_GBN_EVAL leaves in st + 2 co and st + 3 co), 16-byte
 * aligned; res: the residual, a view [b][hout][wout] of co channels with pixel stride ld_res >= co, or NULL with ld_res 0.
 * Bit-identical to ptta_op_gconv with act 0 and the same six_b followed by ptta_op_gbn in mode PTTA_GBN_EVAL with the same act and, with a
 * residual, act_first 0 / res_relu 1 (no flag), act_first 1 / res_relu 1 (ACT_FIRST), act_first 0 / res_relu 0 (RES_PLAIN)
 * (tests/test_gpu_gconv_affine.py, tests/test_gpu_gconv_affine_forms.py).  Matrix-core forms only: impl 0, c0 and c1 multiples of 8
 * (PTTA_GCONV_S1) or 16, act 0 / 1 / 2 (4 as stated above; ptta_op_gconv itself refuses 4), no accumulate, no statistics, no PTTA_GCONV_DGRAD.  six_b as in ptta_op_gconv: the images below it
 * bf16x6, with every form above, on PTTA_GCONV_S1 and every launch form of PTTA_GCONV_S2.  PTTA_GCONV_T2 has the first form in bf16x3 only
 * (no stage-2 prefix holds a transposed layer).  -22 BEFORE any launch for anything else: ACT_FIRST without res or with an activation other
 * than ReLU, RES_PLAIN without res or with an activation, both flags, six_b > b, a NULL or misaligned scale / shift, res without ld_res (or
 * the reverse, or ld_res < co). */
int ptta_op_gconv_affine(const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, const float* weight, const float* bias, float* y,
                         int co, int ldy, int b, int hin, int win, int hout, int wout, int k, int geom, int act, int accumulate, int impl,
                         int flags, int six_b, int x1_from_b, int stat_npass, double* stat_host, int* form_host, const float* scale,
                         const float* shift, const float* res, int ld_res, ptta_stream s);
/* Test hook: ONE BatchNorm of the generic op-list engine (csrc/gbn.hip: every BatchNorm of NLSPN, CostDCNet and the heads, and the apply /
 * backward launchers of the MSG_CHN 2layers block) on caller-supplied fp32 NHWC device views, launched the way the engine's forward and
 * backward sweeps launch it, with the engine's scratch sizes.  A view is a pointer, its channel count and its pixel stride ld >= c;
 * channels outside a view are not touched.  b images of h x w pixels hold npass (1 or 2) equal slices with their own statistics.
 *   PTTA_GBN_TRAIN     x, optional res -> y and st [4][npass][c] = {mean, inv, scale, shift}.  part_in != NULL: caller-made partial sums
 *                      [npass][nblocks_in][2][c] = {sum x, sum x^2} stand in for a convolution epilogue's and the statistics pass is
 *                      skipped.  rm != NULL (with rv; nbt, st_eval optional): a tracked BatchNorm, running statistics updated npass *
 *                      repeats times with `momentum`, st_eval [4][c] = the eval affine of the updated buffers.
 *   PTTA_GBN_EVAL      st [4][c] from rm / rv, then y = the apply with npass = 1.
 *   PTTA_GBN_BACKWARD  x and y over all passes; g, gx and optional gres (its presence says that the forward had a residual) over the
 *                      b / npass images of pass 0; st from the forward.  dgamma / dbeta [c] may be NULL (frozen parameters).
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.2), 4 ELU.  world > 1: a SyncBatchNorm exchange whose collective multiplies the buffer by `world`
 * (every rank holds the same data) -- the collapse / expand kernels, the R * world row count and the 1 / world gradient scale without a
 * communicator.
 * -22 BEFORE any launch for: c not a multiple of 4, ld < c or not a multiple of 4, a view, st or an [n][c] table not 16-byte aligned,
 * views whose channel counts disagree, b not a multiple of npass, and the switch combinations no kernel computes in both directions
 * (residual with res_relu = 0 and act != 0; residual with res_relu = 1, act_first = 1 and act != ReLU).  -12 out of memory.
 * Synchronises. */
#define PTTA_GBN_TRAIN 0
#define PTTA_GBN_EVAL 1
#define PTTA_GBN_BACKWARD 2
typedef struct ptta_gbn_view { float* p; int c; int ld; } ptta_gbn_view;
typedef struct ptta_gbn_args {
    int mode, b, h, w, npass, act, act_first, res_relu, acc_gx, acc_gres, world, nblocks_in, repeats;
    float eps, momentum;
    ptta_gbn_view x, res, y, g, gx, gres;
    const float* gamma; const float* beta; const float* part_in;
    float* st; float* rm; float* rv; long long* nbt; float* st_eval; float* dgamma; float* dbeta;
} ptta_gbn_args;
int ptta_op_gbn(const ptta_gbn_args* a, ptta_stream s);
/* Test hooks: CostDCNet's own kernels (csrc/costdc_kernels.hip) on caller-supplied device buffers, launched through the launchers of
 * csrc/costdc.h exactly as the engine (csrc/costdc_api.hip) launches them.  All of them synchronise; -22 BEFORE any launch for arguments
 * the kernels would index out of bounds with, -12 out of memory, -5 a HIP error.
 *
 * ptta_cd_sparse: the sparse voxel sets of the 3-D encoder for n frames of h x w pixels (h, w multiples of 4: level l has tensor stride
 * (1, 1 << l, 1 << l)), with the scratch the engine gives them.  _build: depth2MDP of `sparse` [n][h][w] (device) and the two coarser
 * levels.  _read: cnt_host [3] voxel counts; of `level`: coords_host [min(cnt, coords_cap)][4] = (frame, plane, y, x), vol_host
 * [n][16][h >> level][w >> level] (voxel id or -1) and, level 0 only, feat_in_host [min(cnt, coords_cap)]; NULL skips an output. */
typedef struct ptta_cd_sparse ptta_cd_sparse;
int ptta_cd_sparse_create(ptta_cd_sparse** out, int n, int h, int w);
void ptta_cd_sparse_destroy(ptta_cd_sparse* q);
int ptta_cd_sparse_build(ptta_cd_sparse* q, const float* sparse, float z_step, ptta_stream s);
int ptta_cd_sparse_read(ptta_cd_sparse* q, int level, int* cnt_host, int* coords_host, long long coords_cap, int* vol_host, float* feat_in_host,
                        ptta_stream s);
/* Generalized sparse convolution from level lin to level lout (lout = lin or lin + 1: stride (1,2,2)), kernel (ksize^3, ci, co), ksize 1 or 3.
 * backward = 0: x [cnt[lin]][ci] -> y [cnt[lout]][co] (co <= 64).  backward = 1: the transpose, x = dy [cnt[lout]][co] -> y = dx [cnt[lin]][ci]
 * (ci <= 64), added to y when acc = 1. */
int ptta_op_cd_sparse_conv(ptta_cd_sparse* q, const float* x, const float* wk, float* y, int lin, int lout, int ksize, int ci, int co, int backward,
                           int acc, ptta_stream s);
/* BatchNorm over the voxels of `level` (c <= 64 channels), mode as ptta_op_gbn's.
 *   PTTA_GBN_TRAIN     f, optional res -> out = relu?(bn(f) + res?) and st [4][c] = {scale, shift, mean, inv}; rm != NULL (with rv; nbt
 *                      optional): running statistics updated `repeats` times (momentum 0.1, unbiased variance).
 *   PTTA_GBN_EVAL      the same from rm / rv.
 *   PTTA_GBN_BACKWARD  f, y (the forward's output), g, st -> gx, dgamma, dbeta and optional gres (written, or added to when acc_res = 1).
 * world > 1: the stand-in collective of ptta_op_gbn (train and backward). */
typedef struct ptta_cd_sbn_args {
    int mode, level, c, relu, repeats, world, acc_res;
    const float* f; const float* res; const float* y; const float* g; const float* gamma; const float* beta;
    float* rm; float* rv; long long* nbt; float* out; float* st; float* dgamma; float* dbeta; float* gx; float* gres;
} ptta_cd_sbn_args;
int ptta_op_cd_sbn(ptta_cd_sparse* q, const ptta_cd_sbn_args* a, ptta_stream s);
/* backward = 0: in [cnt[2]][c] -> out [n][16][h/4][w/4][c] (zero elsewhere).  backward = 1: in = the gradient volume with ldv channels per
 * cell, out [cnt[2]][c] = its channels c0 .. c0 + c - 1 at the level-2 voxels. */
int ptta_op_cd_densify(ptta_cd_sparse* q, const float* in, float* out, int c, int backward, int ldv, int c0, ptta_stream s);
/* The dense kernels.  d = integer arguments, f = float arguments {div, mean[3], std[3]} or {z_step} or {max depth}; a, b inputs, out, out2
 * outputs (NHWC / NDHWC as csrc/costdc_kernels.hip states them):
 *   PAD_DUAL          d {N, C, H, W, Hp, Wp, pt, pr, norm}     a [N][C][H][W] -> out [2N][C][Hp][Wp]; norm = 1 (C = 3) normalises in-frame pixels
 *   CROP_AVG          d {N, H, W, Hp, Wp, pt, pr}              a [2N][Hp][Wp] -> out [N][H][W]   (H + pt <= Hp, W + pr <= Wp)
 *   SCATTER_DUAL_GRAD d {N, H, W, Hp, Wp, pt, pr}              a [N][H][W] -> out [2N][Hp][Wp]
 *   STAGE             d {N, passes, H, W, C, norm}             a image [N][3][H][W], b sparse [N][H][W] -> out [passes N][H][W][C], C 4 or 16
 *   CLAMP             d {n}, f {max depth}                     a -> out
 *   FUSION_FWD        d {N, passes, h, w}                      a feat2d [passes N][h][w][16], b feat3d [N][16][h][w][16] -> out [passes N][16][h][w][32], out2 mask [N][16][h][w]
 *   FUSION_BWD        d {N, h, w}                              a gvol [N][16][h][w][32], b mask -> out [N][h][w][16]
 *   POOL_FWD          d {items_out, H, W, C}                   a [2 items_out][H][W][C] -> out [items_out][H/2][W/2][C], C % 4 == 0
 *   POOL_BWD          d {items_in, H, W, C, acc}               a x, b gy -> out gx; items_in even
 *   UP_FWD            d {frames, Di, Hi, Wi, Do, Ho, Wo, C}    a -> out, C % 4 == 0
 *   UP_BWD            d {frames, Di, Hi, Wi, Do, Ho, Wo, C, acc}  a gy -> out gx
 *   REGRESS_FWD       d {N, h, w}, f {z_step}                  a cost [N][16][h][w][16] -> out [N][4h][4w]
 *   REGRESS_BWD       d {N, h, w}, f {z_step}                  a cost, b gpred -> out gcost
 *   ROWS_FWD          d {N, D, h, w, C}                        a [N][D][h][w][C] -> out [N h w][C D]
 *   ROWS_BWD          d {N, D, h, w, C, acc}                   a grows -> out gfeat
 * Buffers a kernel reads or writes as float4 must be 16-byte aligned. */
#define PTTA_CD_PAD_DUAL 0
#define PTTA_CD_CROP_AVG 1
#define PTTA_CD_SCATTER_DUAL_GRAD 2
#define PTTA_CD_STAGE 3
#define PTTA_CD_CLAMP 4
#define PTTA_CD_FUSION_FWD 5
#define PTTA_CD_FUSION_BWD 6
#define PTTA_CD_POOL_FWD 7
#define PTTA_CD_POOL_BWD 8
#define PTTA_CD_UP_FWD 9
#define PTTA_CD_UP_BWD 10
#define PTTA_CD_REGRESS_FWD 11
#define PTTA_CD_REGRESS_BWD 12
#define PTTA_CD_ROWS_FWD 13
#define PTTA_CD_ROWS_BWD 14
int ptta_op_cd_dense(int op, const float* a, const float* b, float* out, float* out2, const int* d, const float* f, ptta_stream s);
/* Test hooks: the MSG_CHN step's first-layer / prediction convolutions (csrc/conv_small.hip), resamplings (csrc/resample.hip) and loss
 * (csrc/loss.hip) on caller-supplied fp32 device buffers, packed and launched through the launchers of csrc/ptta_kernels.h exactly as
 * csrc/msgchn_forward.hip, msgchn_backward.hip and msgchn_step.hip launch them (tests/test_gpu_msgchn_elementwise.py).  All of them
 * synchronise; -22 BEFORE any launch (and before any allocation) for arguments a kernel would index out of bounds or misalign with, -12 out
 * of memory, -5 a HIP error.  dtype other than PTTA_DTYPE_F32: the 32-channel maps are converted to narrow (bf16) storage and back, as
 * ptta_op_conv32 does; planar one-channel maps stay fp32 in both modes.
 *
 * ptta_op_conv_in: planar planes pl[0 .. cin) (each [nb][h][w], frame b % nb, optional normalisation (v / div - mean) / stdv of in-frame
 * samples) -> 32-channel NHWC.  weight as the state dict holds it, [32][cin_total][3][3] from input channel cin_first on, or with
 * transpose_flip the [1][32][3][3] weight of a 32 -> 1 convolution packed as its input gradient (cin 1).  Epilogue, each operand optional:
 * bias [32]; up [up_nb][h/2][w/2][32] (bilinear x2, h and w even); ReLU mask as a float map mask [mask_nb][h][w][32] and / or sign-bit
 * words mask_bits [mask_nb][h][w]; add1 [add1_nb][h][w][32] (goes into out_sum only).  out_raw / out_sum [b][h][w][32] (either may be NULL,
 * not both; a NULL one is not written); a_bits [b][h][w]: the sign-bit words of out_raw for frames below a_bits_nb.  Frames from
 * zero_from_b on see a zero input (the proxy pass).  max_blocks > 0 caps the grid.  *form_host: the kernel that ran -- 0 LDS-staged,
 * 1 LDS-staged with mask, 2 the direct matrix-core form (taken with up or add1), 3 naive.  Refused: a narrow launch with a float mask and
 * no bit words; bit words without a float mask in the direct and naive forms, or any mask there in a narrow launch (those kernels read the
 * map); a_bits outside the fp32 LDS-staged forms (nothing else writes them). */
typedef struct ptta_plane { const float* p; int nb; int norm; float div, mean, stdv; } ptta_plane;
typedef struct ptta_conv_in_args {
    int cin, cin_total, cin_first, transpose_flip, up_nb, mask_nb, add1_nb, a_bits_nb, zero_from_b, b, h, w, dtype, naive, max_blocks;
    ptta_plane pl[3];
    const float* weight; const float* bias; const float* up; const float* mask; const uint32_t* mask_bits; const float* add1;
    float* out_raw; float* out_sum; uint32_t* a_bits;
} ptta_conv_in_args;
int ptta_op_conv_in(const ptta_conv_in_args* a, int* form_host, ptta_stream s);
/* ptta_op_conv_out1: in [in_nb][h][w][32] (frame b % in_nb, ReLU on load with relu_in) -> out [b][h][w] = conv + bias[0] + add[b % add_nb]
 * (bias, add may be NULL).  weight [1][32][3][3], or with from_conv_in the [32][src_cin_total][3][3] weight of a first layer packed as the
 * input gradient with respect to its plane src_cin_index.  max_blocks > 0 caps the grid. */
typedef struct ptta_conv_out1_args {
    int in_nb, src_cin_total, src_cin_index, from_conv_in, add_nb, relu_in, dtype, b, h, w, max_blocks;
    const float* in; const float* weight; const float* bias; const float* add; float* out;
} ptta_conv_out1_args;
int ptta_op_conv_out1(const ptta_conv_out1_args* a, ptta_stream s);
/* ptta_op_prep: sparse [n][h][w] -> dclamp (clamped to [0, max_input_depth]; max_input_depth < 0: a copy), d12 [n][h/2][w/2] and d14
 * [n][h/4][w/4] = avg_pool(d) / (avg_pool(d > 0) + 1e-4).  h, w multiples of 4 (else -22).
 * ptta_op_up2_1ch: in [b][hin][win] -> out [b][2 hin][2 win], bilinear x2 with align_corners; ptta_op_up2t_1ch its transpose, gout
 * [b][2 hin][2 win] -> gin [b][hin][win]; ptta_op_up2t_32 the transpose on 32-channel NHWC maps, gin = add + up2^T(gout) (add may be NULL). */
int ptta_op_prep(const float* sparse, float max_input_depth, float* dclamp, float* d12, float* d14, int n, int h, int w, ptta_stream s);
int ptta_op_up2_1ch(const float* in, float* out, int b, int hin, int win, ptta_stream s);
int ptta_op_up2t_1ch(const float* gout, float* gin, int b, int hin, int win, ptta_stream s);
int ptta_op_up2t_32(const float* gout_nhwc, const float* add_nhwc, float* gin_nhwc, int b, int hin, int win, int dtype, ptta_stream s);
/* ptta_op_loss: the adaptation loss and its gradients, every launch form.  depth, sparse, validity (NULL: where(sparse > 0, 1, sparse))
 * [n][h][w], image [n][3][h][w], emb / ref [r][d] (both or neither), the weights w_sd, w_sm, w_cos.  The workspace has
 * the size the engine gives it (csrc/loss.hip) and starts NaN-filled.
 *   fwd  PTTA_LOSS_FWD_MERGED   ptta_launch_loss_forward with emb and ref: the merged reduction + the finalisation
 *        PTTA_LOSS_FWD_NOCOS    ptta_launch_loss_forward without the cosine term (emb, ref ignored)
 *        PTTA_LOSS_FWD_SPLIT    loss_depth_part + loss_cos_part + loss_finalize (the fused step's branches); _SPLIT_NARROW: bf16 embeddings
 *   bwd  PTTA_LOSS_BWD_NONE
 *        PTTA_LOSS_BWD_UNFUSED  the separate depth and cosine gradient kernels reading the finalised workspace
 *        PTTA_LOSS_BWD_FUSED    the forward launched with its finalisation deferred, then the gradient launch that finalises inside its
 *                               kernels (merged depth + cosine kernel with emb and ref; fwd _MERGED or _NOCOS)
 *        PTTA_LOSS_BWD_COUNTED  the thru step: loss_valid_count, loss_cos_part (fwd _SPLIT / _SPLIT_NARROW), loss_cos_coef, the depth
 *                               gradient from the valid-weight partials, then the loss values (loss_depth_part + loss_finalize) and the
 *                               cosine gradient kernel reading the coefficient from the workspace
 * Outputs (each may be NULL): loss_info [4]; rowstats [r][3] = (|e|, |ref|, cos); gdepth [n][h][w]; gref [r][d]; coef [4 + n] =
 * {coef_cos, coef_smx, coef_smy, n per-sample sparse-depth coefficients} read back from the workspace after the last launch, and in
 * [3 + n] what loss_cos_coef alone left in the workspace (_COUNTED; untouched otherwise).
 * -22: d not a multiple of 4 (8 for narrow embeddings), h < 2 or w < 2 (the smoothness counts divide by h - 1 and w - 1), r < 1 with a
 * cosine term, a form combination outside the list above. */
#define PTTA_LOSS_FWD_MERGED 0
#define PTTA_LOSS_FWD_NOCOS 1
#define PTTA_LOSS_FWD_SPLIT 2
#define PTTA_LOSS_FWD_SPLIT_NARROW 3
#define PTTA_LOSS_BWD_NONE 0
#define PTTA_LOSS_BWD_UNFUSED 1
#define PTTA_LOSS_BWD_FUSED 2
#define PTTA_LOSS_BWD_COUNTED 3
typedef struct ptta_loss_args {
    int fwd, bwd, n, h, w, d;
    long long r;
    float max_input_depth, w_sd, w_sm, w_cos;
    const float* depth; const float* image; const float* sparse; const float* validity; const float* emb; const float* ref;
    float* loss_info; float* rowstats; float* gdepth; float* gref; float* coef;
} ptta_loss_args;
int ptta_op_loss(const ptta_loss_args* a, ptta_stream s);
/* Test hooks: NLSPN's propagation gradients stand-alone, in both forms (csrc/nlspn_prop.hip; option "deterministic").  Planar fp32 device maps:
 * pinned, fix, gout, gfeat [b][h*w]; off9, goff9 [b][18][h*w]; aff9, gaff9 [b][9][h*w].  form 0: the float-atomic kernels of the default step;
 * form 1: the fixed-point forms, with the maxima their scale comes from reduced from aff9 and gout first, as the engine's backward does.
 * scratch: ptta_nl_det_scratch_bytes(b, h, w) bytes of device memory, 8-byte aligned (form 1; form 0 takes NULL) -- 256 + 8 * b * h * w.
 * ptta_op_nl_prop_bwd: ONE sweep's gradient: gfeat is overwritten, goff9 and gaff9 are accumulated into (the engine adds 18 sweeps).  reps > 0:
 * `reps` more launches of the sweep (form 0: its memset and kernel; form 1: scatter and convert) timed with hipEvents on s, microseconds per
 * sweep to *us_per_call_host -- goff9 / gaff9 keep accumulating.  ptta_op_nl_affinity_bwd: oa and goa are CONTIGUOUS NHWC maps of 24 channels
 * (o1 | o2 | aff), aff_scale one device float (prop_layer.aff_scale_const), legacy 0 / 1 (PTTA_NLSPN_LEGACY_OFFSET); goa and gconf [b][h*w] are
 * overwritten.  Both synchronise. */
int64_t ptta_nl_det_scratch_bytes(int b, int h, int w);
int ptta_op_nl_prop_bwd(const float* pinned, const float* fix, const float* off9, const float* aff9, const float* gout, float* gfeat,
                        float* goff9, float* gaff9, int b, int h, int w, int form, void* scratch, int reps, float* us_per_call_host,
                        ptta_stream s);
int ptta_op_nl_affinity_bwd(const float* oa_nhwc, const float* conf, const float* aff_scale, int legacy, const float* goff9, const float* gaff9,
                            float* goa_nhwc, float* gconf, int b, int h, int w, int form, void* scratch, ptta_stream s);
/* Test hooks: the narrow heads of the mixed mode (csrc/heads_n.hip) and head_bwd_finish (csrc/heads_bn.hip) stand-alone, launched through
 * the launchers of csrc/ptta_kernels.h (tests/test_gpu_heads_n_elementwise.py).  All of them synchronise; -12 out of memory, -5 a HIP error.
 *
 * Layouts.  A narrow [R][512] activation is TILED: T[r / 128][k / 32][r % 128][k % 32] bf16, ptta_op_hn_tiled_elems(R) = ceil(R / 128) * 128 *
 * 512 elements -- the rows from R on of the last block are padding: the GEMM reads them (their results land in the output's padding) and no
 * result of a row below R depends on them.  part [ceil(R / 128)][2][512] fp32: per 128-row block the column sums (epi 1: sum v | sum v^2
 * of the fp32 values; epi 3: sum g | sum g xhat of the masked gradient), rows below R only.  rs [R]: row sums of squares of the STORED
 * values.  rowstats / rowstats_out [R][3] = (|e|, |c|, cos), both norms floored at 1e-12.  cpart [cpart_n]: slot b < ceil(R / 128) = block
 * b's sum of 2 - 2 cos over its rows below R, the slots from ceil(R / 128) on are cleared.  P [R][32] fp32.
 *
 * ptta_op_hn_gemm: one field per field of HnGemmArgs, passed through to the launcher ptta_launch_hn_gemm; -22 exactly where that returns -22: W NULL,
 * r < 1, a pointer its pro / epi needs NULL, cpart_n below the grid, a key other than 10 11 12 30 31 35 43 53.  A, Bref, E, C: device buffers
 * in the tiled layout.  W [512][512], W0 [512][32], W0t [32][512] arrive as fp32 row-major and are converted inside the call the way
 * csrc/msgchn_build.hip converts them: ptta_split_weight's hi plane, then ptta_hn_pack_w for W; w_image (may be NULL) receives the packed
 * slice-major image of W, [16][512][32] bf16 with 16-byte chunk c of row n at c ^ ((n >> 2) & 3).  Scratch is allocated and freed inside.
 * ptta_op_hn_moments: ptta_launch_hn_moments on X [npass][r][32] (fp32, or bf16 with x_bf16), W0 [512][32] and b0 fp32 -> part [npass][2][2][512]
 * (sum h | sum h^2 as a float value and the remainder its rounding lost), or with bn != 0 the BatchNorm1d state directly: gamma, beta in;
 * mean, inv, scale, shift [512] out; rm, rv (both or neither), nbt optional.  -22 where the launcher returns it (a NULL input, r < 1,
 * npass < 1, bn with npass != 1) and for bn with gamma, beta, mean, inv, scale or shift NULL or rm without rv (the kernel would dereference them).
 * ptta_op_hn_untile: tiled bf16 -> dst [r][512] fp32.  ptta_op_head_bwd_finish: dX [r][32] (fp32, or bf16 with dx_bf16) = P - X M - u with
 * M, u from k12 [2][512] doubles and W0 [512][32] fp32 (csrc/heads_bn.hip); P [halves][r][32], halves 1 or 2 (else -22). */
long long ptta_op_hn_tiled_elems(long long r);      /* elements of a tiled [r][512] buffer; -22 for r < 1 */
typedef struct ptta_hn_gemm_args {
    int pro, epi, x_bf16, cpart_n;
    long long r;
    const void* A; const float* Af; const void* Bref; const float* rowstats; const float* coef; const void* X;
    const float* W0; const float* b0; const float* pscale; const float* pshift; const float* W; const float* bias;
    void* C; float* part; const void* E; float* rs; float* rowstats_out; float* cpart;
    const float* escale; const float* eshift; const float* emean; const float* einv; const float* W0t; float* P;
    void* w_image;
} ptta_hn_gemm_args;
int ptta_op_hn_gemm(const ptta_hn_gemm_args* a, ptta_stream s);
typedef struct ptta_hn_moments_args {
    int x_bf16, npass, bn;
    long long r;
    float eps, momentum;
    const void* X; const float* W0; const float* b0; float* part;
    const float* gamma; const float* beta; float* rm; float* rv; long long* nbt; float* mean; float* inv; float* scale; float* shift;
} ptta_hn_moments_args;
int ptta_op_hn_moments(const ptta_hn_moments_args* a, ptta_stream s);
int ptta_op_hn_untile(const void* src_tiled, float* dst, long long r, ptta_stream s);
int ptta_op_head_bwd_finish(const double* k12, const float* W0, const float* P, const float* X, long long r, void* dX, int halves, int dx_bf16,
                            ptta_stream s);
/* Test hooks: the update half of a step stand-alone -- weight gradients and the optimizer -- launched through the launchers of
 * csrc/ptta_kernels.h (csrc/ptta_ops_update.hip; tests/test_gpu_update_elementwise.py).  Every pointer is device memory unless it says
 * host.  Partial buffers and device tables are allocated and freed inside the call.  All of them synchronise; -12 out of memory, -5 a HIP
 * error.  The launchers dereference what they are given, so every hook refuses (-22) a NULL required pointer and a size below 1 before its
 * first launch; past that it returns -22 exactly where its launcher does.
 *
 * ptta_op_wgrad32 (ptta_launch_wgrad32: wgrad32_kernel<float> / <bf16> + wgrad32_reduce_kernel): weight and bias gradient of a stride-1 3x3
 * convolution of 32 -> 32 channels, zero padding 1.  x, gy: dense NHWC maps [b][h][w][32], both fp32 or (bf16 != 0) both bf16.  gw: element
 * (co, ci, tap) at gw[co * co_stride + ci * 9 + tap], tap = 3 ky + kx -- co_stride = 288 is a dense [32][32][3][3] weight, 9 * Ci a group of
 * 32 input channels inside a [32][Ci][3][3] weight (pass gw already offset by 9 * first channel); the other elements are not touched.
 * gb [32] or NULL.  The launcher itself refuses nothing; -22 from the hook: co_stride < 288, b * h * w * 32 above 2e9 elements.
 *
 * ptta_op_gwgrad_view (ptta_launch_gwgrad_mfma): the same gradient for ci -> co channels on strided views.  x: fp32, pixel stride ldx >= ci
 * ELEMENTS, the pointer already offset to the view's first channel; gy likewise with ldg >= co, fp32 or (gy_bf16) bf16 elements.  gw
 * [co][ci][3][3] dense, gb [co] or NULL.  Adam inside the reduction when pw != NULL: pw, mw, vw [co][ci][3][3] and, unless pb == NULL, pb,
 * mb, vb [co]; hyper = {lr, beta1, beta2, eps, weight_decay} fp32; step one int (the count BEFORE this update; the call leaves step + 1);
 * ticket one unsigned that is 0 and comes back 0.  -22 from the launcher: gy_bf16 at a shape without a bf16x3 form that takes bf16
 * gradients (the forms: ci, co <= 64, or ci <= 32 and co <= 128, or ci <= 128 and co <= 32, each with ci > 16); an Adam block at anything
 * but ci, co <= 32 with ci > 16.  -22 from the hook: ci or co above 256, ldx < ci, ldg < co, pw with mw, vw, hyper, step or ticket NULL,
 * pb with mb or vb NULL.
 *
 * ptta_op_adam = ptta_launch_step_inc + ptta_launch_adam, the launcher of adam_kernel, as ptta_adam_step with explicit gradients: step becomes step + 1,
 * then p, m, v [n] are updated with g [n] at that count.  ptta_op_adam_multi (ptta_launch_adam_multi: adam_multi_kernel) and
 * ptta_op_ema_multi (ptta_launch_ema_multi: ema_multi_kernel) take HOST arrays of nt device pointers and sizes; the hook lays them out as
 * the device PttaAdamEntry table with running offsets.  rep[k] (host; NULL = all 1): 0 = listed but without a gradient (p, m, v, g of that
 * entry are not read or written), r > 1 = r consecutive updates with the same gradient at the counts (t - 1) r + 1 .. t r.  The launch
 * leaves step + 1 and ticket 0.  ptta_op_ema_multi: p[k] = fl(fl(p[k] tau) + fl(g[k] omt)) with tau_dev = {tau, omt} two device floats.
 * -22: nt < 1, n[k] < 1, rep[k] < 0, a NULL pointer of an entry with rep != 0 (g may not be NULL for rep != 0).
 *
 * ptta_op_linear_wgrad (ptta_launch_linear_wgrad: linear_wgrad_kernel<NT, GPRO, XPRO> + wgrad_reduce_kernel): dW [O][I] = sum_r G'[r][o]
 * X'[r][i], db [O] (may be NULL) = sum_r G'[r][o] over dense row-major G [R][O], X [R][I].  Gh != NULL (GPRO): G' = gscale (G - gc1 -
 * (Gh - gmean) ginv gc2), the BatchNorm-backward transform with per-column tables [O]; xscale != NULL (XPRO): X' = relu(X xscale + xshift),
 * tables [I].  -22 from the launcher: O % 128 != 0, I neither 32 nor a multiple of 128, R < 1, xscale with I = 32.  -22 from the hook: O < 1 or
 * I < 1, Gh with a NULL table, xscale without xshift.
 * ptta_op_glinear_wgrad (ptta_launch_glinear_wgrad: glinear_wgrad_kernel): gw [O][I] = sum_r gy[r][o] x[r][i], gb [O] or NULL, x [R][ldx]
 * with ldx >= I and gy [R][ldg] with ldg >= O, fp32, any I, O >= 1.  -22 from the launcher: R < 1, gw NULL; from the hook: I < 1, O < 1,
 * ldx < I, ldg < O, R above 2e9 (the launcher's views count rows in an int). */
int ptta_op_wgrad32(const void* x_nhwc, const void* gy_nhwc, int bf16, int b, int h, int w, float* gw, float* gb, int co_stride, ptta_stream s);
typedef struct ptta_gwgrad_view_args {
    int b, h, w, ci, co, ldx, ldg, gy_bf16;
    const float* x; const void* gy; float* gw; float* gb;
    float* pw; float* mw; float* vw; float* pb; float* mb; float* vb; const float* hyper; int* step; unsigned* ticket;
} ptta_gwgrad_view_args;
int ptta_op_gwgrad_view(const ptta_gwgrad_view_args* a, ptta_stream s);
int ptta_op_adam(float* p, float* m, float* v, const float* g, long long n, const float* hyper, int* step, ptta_stream s);
int ptta_op_adam_multi(int nt, float* const* p, float* const* m, float* const* v, const float* const* g, const long long* n, const int* rep,
                       const float* hyper, int* step, unsigned* ticket, ptta_stream s);
int ptta_op_ema_multi(int nt, float* const* p, const float* const* g, const long long* n, const float* tau_dev, ptta_stream s);
typedef struct ptta_linear_wgrad_args {
    long long r;
    int o, i;
    const float* G; const float* Gh; const float* gscale; const float* gc1; const float* gc2; const float* gmean; const float* ginv;
    const float* X; const float* xscale; const float* xshift; float* dW; float* db;
} ptta_linear_wgrad_args;
int ptta_op_linear_wgrad(const ptta_linear_wgrad_args* a, ptta_stream s);
int ptta_op_glinear_wgrad(const float* x, int ldx, int i, const float* gy, int ldg, int o, long long r, float* gw, float* gb, ptta_stream s);
/* Diagnostic (tools/bench_chain.py): `reps` dependent launches of one stride-1 32->32 convolution (fp32 NHWC, default arithmetic) captured
 * into one hipGraph and replayed `replays` times: microseconds per launch INSIDE a replayed graph.  epi_flags: 2 = ReLU mask from `aux`,
 * 4 = skip addition of `aux`, 8 = the same chain launched directly (no graph), 16 = the layer loop (ONE launch per `reps` layers with a
 * device-wide barrier between layers; plain epilogue only; -62 when a bounded barrier spin ran out).  Synchronises. */
int ptta_op_conv32_chain(const float* in_nhwc, const float* weight, const float* bias, float* buf_a, float* buf_b, const float* aux,
                         int b, int h, int w, int relu_in, int epi_flags, int reps, int replays, float* us_per_launch_host, ptta_stream s);
/* ABI version of this header: ptta_version() of a loaded library must equal the PTTA_ABI_VERSION the binding was written against
 * (proxytta/_lib.py checks it at load).  2: ptta_step_pipelined takes the next frame's pointers; ptta_set_option / ptta_get_option;
 * PTTA_DTYPE_MIXED replaces the bf16 storage mode. */
#define PTTA_ABI_VERSION 2
int ptta_version(void);

#ifdef __cplusplus
}
#endif
#endif
