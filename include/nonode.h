/*
 * nonode.h — C ABI of the MI355X-native EGNO / SEGNO trajectory-rollout hot path.
 *
 * Drop-in boundary for simone7monaco/NO-NODE-comparison (reference @ 2025-07-04).
 * The reference has no FFI of its own: its boundary is the pair of torch.nn.Module
 * classes EGNO (EGNO/model/egno.py:8-111) and SEGNO (SEGNO/models/model.py:6-102).
 * These entry points are what the Python mirror of those classes (package
 * no-node-comparison_amd, loaded through ctypes) binds; INTEGRATION.md shows the
 * binding. Every pointer is a DEVICE pointer unless the comment says "host";
 * every call is asynchronous on `stream` (a hipStream_t passed as void*), never
 * allocates, never synchronises, and returns 0 on success or a nonzero
 * nonode_status (the reason is in nonode_last_error()).
 *
 * Layouts (fp32, row-major, no padding):
 *   node arrays     [n_nodes][C]; EGNO nodes are time-major: row = t*B*N + b*N + n
 *   edge features   [n_graphs_ef * N*(N-1)][n_edge_feat] in the reference edge order
 *                   (b, i, j != i)  (EGNO/simulation/dataset_simple.py:64-71,101-111)
 *   graphs          fully connected, equal size N, no self loops; row = receiver i,
 *                   col = sender j (basic.py:168-186, gcl.py:111-119). The *_graph entries at the
 *                   end take any edge list instead, as a CSR by receiver (inference; EGNO training:
 *                   nonode_egnn_layer_graph_bwd).
 */
#ifndef NONODE_H_
#define NONODE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  NONODE_OK = 0,
  NONODE_EINVAL = 1,       /* bad argument (shape, null pointer, unsupported size) */
  NONODE_ELAUNCH = 2,      /* HIP launch / runtime error */
  NONODE_EUNSUPPORTED = 3  /* configuration outside what the kernels implement */
} nonode_status;

/* Variant of the shared E(n)-equivariant layer. */
enum { NONODE_VARIANT_EGNO = 0, NONODE_VARIANT_SEGNO = 1 };
/* Option bits OR-ed into the variant of nonode_pack_layer / nonode_pack_layer_bwd (stored in the
 * blob, so every forward, backward and rollout entry that takes the blob follows them):
 *  NORM_RADIAL: EGNO(norm=True): the radial edge input is F.normalize(|x_i - x_j|^2) over its one
 *               element = s / max(s, 1e-12) (InvariantScalarNet, basic.py:136-141);
 *  TANH_COORD:  SEGNO(tanh=True): the coordinate MLP ends in nn.Tanh (gcl.py:57-59). */
enum { NONODE_LAYER_NORM_RADIAL = 0x100, NONODE_LAYER_TANH_COORD = 0x200 };

const char* nonode_version(void);
/* Thread-local message describing the last nonzero status. */
const char* nonode_last_error(void);

/*
 * Raw nn.Linear parameters of ONE layer, exactly as stored in the reference state_dict.
 *  EGNO  EGNN_Layer (EGNO/model/basic.py:147-165):
 *    edge_w1/b1 = edge_message_net.scalar_net.mlp.0  [64][1+64+64+E] input order [s,h_i,h_j,e]
 *    edge_w2/b2 = edge_message_net.scalar_net.mlp.2  [64][64]
 *    coord_*    = coord_net.mlp.{0,2}                [64][64], [1][64]
 *    vel_*      = node_v_net.mlp.{0,2}               [64][64], [1][64]
 *    node_*     = node_net.mlp.{0,2}                 [64][128], [64][64]
 *  SEGNO SEGNO_GCL (SEGNO/models/models/gcl.py:26-69):
 *    edge_w1/b1 = edge_mlp.0  [64][64+64+1+E] input order [h_i,h_j,s,e]
 *    edge_w2/b2 = edge_mlp.2, coord_* = coord_mlp.{0,2}, node_* = node_mlp.{0,2};
 *    vel_* unused (pass NULL; coord_mlp_vel is dead in the reference forward).
 */
typedef struct {
  const float* edge_w1; const float* edge_b1;
  const float* edge_w2; const float* edge_b2;
  const float* coord_w1; const float* coord_b1;
  const float* coord_w2; const float* coord_b2;
  const float* vel_w1; const float* vel_b1;
  const float* vel_w2; const float* vel_b2;
  const float* node_w1; const float* node_b1;
  const float* node_w2; const float* node_b2;
} nonode_layer_weights;

/* Floats in one packed layer blob (MFMA fragment order). */
size_t nonode_layer_blob_floats(void);

/* Pack one layer's weights into the kernel's fragment layout (device -> device).
 * Replaces nothing in the reference (weights are read in place by nn.Linear there);
 * call it again after every optimizer step. hidden must be 64, n_edge_feat <= 4. */
int nonode_pack_layer(const nonode_layer_weights* w, int variant, int hidden, int n_edge_feat,
                      float* blob, void* stream);
/* nonode_pack_layer of n_layers layers in one launch (w, blobs: host arrays; same rules per layer).
 * A training step re-packs every layer after each optimizer step (egno.py _packed). */
int nonode_pack_layers(const nonode_layer_weights* const* w, int n_layers, int variant, int hidden,
                       int n_edge_feat, float* const* blobs, void* stream);

/* Workspace bytes nonode_egno_forward needs. */
size_t nonode_egno_workspace_bytes(int B, int N, int T, int Bt);

/*
 * EGNO.forward (EGNO/model/egno.py:37-111) for num_inputs == 1, with_v=True, norm=False,
 * flat=False, use_time_conv=True, hidden 64.
 *   x, v, loc_mean [B*N][3]; h [B*N][in_node]; edge_fea [B*N*(N-1)][n_edge_feat];
 *   t_out [Bt][T] (float; row b' feeds node rows r with r % Bt == b', egno.py:66);
 *   emb_w [64][in_node+time_emb_dim], emb_b [64];
 *   blobs[l]   (host array of device ptrs) packed layers from nonode_pack_layer(EGNO);
 *   tconv_blobs[l] (host array) time_conv_modules.l.t_conv.weights1 packed by nonode_pack_tconv;
 *   tconvx_w[l](host array) time_conv_x_modules.l.t_conv.weights1 [2][2][modes][2];
 *   tconv_blobs = tconvx_w = NULL: EGNO(use_time_conv=False) (egno.py:99-107 skipped; loc_mean
 *   and modes are then unused and loc_mean may be NULL);
 *   outputs x_out, v_out [T*B*N][3], h_out [T*B*N][64] (time-major, egno.py:89-96).
 * Limits: N >= 2, T <= 16, modes <= 9, time_emb_dim even <= 64, in_node <= 8.
 */
int nonode_egno_forward(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                        int time_emb_dim, int modes, int Bt,
                        const float* x, const float* h, const float* v, const float* loc_mean,
                        const float* edge_fea, const float* t_out,
                        const float* emb_w, const float* emb_b,
                        const float* const* blobs, const float* const* tconv_blobs,
                        const float* const* tconvx_w,
                        float* x_out, float* v_out, float* h_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/*
 * EGNO.forward for num_inputs > 1 (EGNO/model/egno.py:44-96 multi-input branch): the same
 * computation as nonode_egno_forward with the inputs already spread over the T frames the way
 * repeat_elements_to_exact_shape (EGNO/utils.py:115-131) does it:
 *   x, v, loc_mean [T*B*N][3]; h [T*B*N][in_node]; edge_fea [T*B*N*(N-1)][n_edge_feat] (frame-major);
 *   t_in [Bt][T] (input time of each frame's input; NULL = single-input embedding), t_out [Bt][T];
 *   emb_w [64][in_node + 2*time_emb_dim] (columns [h | temb(t_in) | temb(t_out)]) when t_in != NULL.
 * Workspace: nonode_egno_workspace_bytes(B, N, T, Bt). Other arguments as nonode_egno_forward.
 */
int nonode_egno_forward_frames(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                               int time_emb_dim, int modes, int Bt,
                               const float* x, const float* h, const float* v, const float* loc_mean,
                               const float* edge_fea, const float* t_in, const float* t_out,
                               const float* emb_w, const float* emb_b,
                               const float* const* blobs, const float* const* tconv_blobs,
                               const float* const* tconvx_w,
                               float* x_out, float* v_out, float* h_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- EGNO(flat=True) (main_simulation_simple_no.py --flat; basic.py:38-40: every BaseMLP 4x wide,
 * 256 hidden channels, with Tanh): forward only ---- */
/* Floats in one packed flat-layer blob. */
size_t nonode_flat_blob_floats(void);
/* Pack one flat EGNN_Layer (variant NONODE_VARIANT_EGNO, optionally | NONODE_LAYER_NORM_RADIAL; hidden 64,
 * so edge W1 [256][129 + ne], W2 [64][256], coord / node_v W1 [256][64], W2 [1][256], node W1
 * [256][128], W2 [64][256]) into the flat layer kernels' fragment layout (device -> device). */
int nonode_pack_layer_flat(const nonode_layer_weights* w, int variant, int hidden, int n_edge_feat,
                           float* blob, void* stream);
/* Workspace bytes nonode_egno_forward_flat needs (nonode_egno_workspace_bytes plus n x 580 floats for
 * the flat layer's node projections and sums, n = B N T). */
size_t nonode_egno_flat_workspace_bytes(int B, int N, int T, int Bt);
/* EGNO.forward with flat=True: the arguments of nonode_egno_forward_frames with blobs from
 * nonode_pack_layer_flat; t_in = NULL takes the single-input layout of nonode_egno_forward
 * (x, v, loc_mean, h, edge_fea of the B N nodes, broadcast over the frames). */
int nonode_egno_forward_flat(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                             int time_emb_dim, int modes, int Bt,
                             const float* x, const float* h, const float* v, const float* loc_mean,
                             const float* edge_fea, const float* t_in, const float* t_out,
                             const float* emb_w, const float* emb_b,
                             const float* const* blobs, const float* const* tconv_blobs,
                             const float* const* tconvx_w,
                             float* x_out, float* v_out, float* h_out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Workspace bytes nonode_segno_forward_step needs. */
size_t nonode_segno_workspace_bytes(int B, int N);

/*
 * SEGNO.embedding + SEGNO.forward_step (SEGNO/models/model.py:73,95-102): h = Linear(his),
 * then T substeps of SEGNO_GCL.forward (gcl.py:111-119) with dt = 1/T, recurrent=True,
 * tanh=False, attention=False, the per-edge clamp(+-100) and the segment mean.
 *   his [B*N][in_node]; x, v [B*N][3]; edge_attr [B*N*(N-1)][n_edge_feat] (frozen over the
 *   substeps, as in the reference); blob from nonode_pack_layer(SEGNO).
 *   h_in: if non-NULL, used as the already-embedded h [B*N][64] and emb_w/his are ignored.
 *   recurrent: h <- h + node_mlp(.) (gcl.py:93-94) when nonzero.
 *   outputs x_out, v_out [B*N][3], h_out [B*N][64].
 */
int nonode_segno_forward_step(int B, int N, int T, int in_node, int n_edge_feat,
                              const float* his, const float* h_in, const float* x, const float* v,
                              const float* edge_attr, const float* emb_w, const float* emb_b,
                              const float* blob, float coords_weight, int recurrent,
                              float* x_out, float* v_out, float* h_out,
                              void* workspace, size_t workspace_bytes, void* stream);

/*
 * Building blocks (the forwards above are sequences of these).
 */
/* Floats of one packed TimeConv weight blob; 0 if modes is unsupported. */
size_t nonode_tconv_blob_floats(int modes);

/* Pack time_conv_modules.l.t_conv.weights1 [64][64][modes][2] (layer_no.py:203-205) for trajectory
 * length T: the irfft scale (c_m / T) is folded in. Call again after every optimizer step. */
int nonode_pack_tconv(const float* tconv_w, int modes, int T, float* blob, void* stream);
/* nonode_pack_tconv of n_layers weight arrays in one launch (tconv_w, blobs: host arrays of device
 * pointers; same rules). */
int nonode_pack_tconvs(const float* const* tconv_w, int n_layers, int modes, int T, float* const* blobs,
                       void* stream);

/* TimeConv + TimeConv_x of one EGNO layer (layer_no.py:96-126,152-178, egno.py:100-108) on
 * time-major [T][BN] arrays; x_out/v_out may alias x/v (in place per column), h_out may not
 * alias h. tconv_blob from nonode_pack_tconv, tconvx_w raw [2][2][modes][2]. */
int nonode_egno_tconv(int BN, int T, int modes, const float* h, const float* x, const float* v,
                      const float* loc_mean, const float* tconv_blob, const float* tconvx_w,
                      float* h_out, float* x_out, float* v_out, void* stream);

/* One fused E(n)-equivariant layer over n_graphs fully connected graphs of N nodes:
 * EGNN_Layer.forward (basic.py:167-186) for variant EGNO, SEGNO_GCL.forward (gcl.py:111-119)
 * for variant SEGNO. Edge features of graph g come from sample g % ef_mod.
 * dt: SEGNO integrator step 1/n_layers (ignored for EGNO). v_out: SEGNO only. */
int nonode_egnn_layer(int variant, int n_graphs, int N, int n_edge_feat, int ef_mod,
                      const float* h, const float* x, const float* v, const float* edge_fea,
                      const float* blob, float dt, float coords_weight, int recurrent,
                      float* h_out, float* x_out, float* v_out, void* stream);

/*
 * Launch timing for benchmarks (not part of the reference boundary). After
 * nonode_profile_begin(n), the next n kernel launches of egnn_layer (kind 0 = EGNO, 1 = SEGNO)
 * and tconv (kind 2, 3 = first layer with embedding) are bracketed by hipEvents recorded on
 * their own stream. nonode_profile_end synchronises those events, writes each launch's duration
 * in ms and its kind, stops recording, and returns the number of records (or < 0 on error).
 */
int nonode_profile_begin(int max_records);
int nonode_profile_end(float* ms_out, int* kind_out, int max_out);

/* ---- EGNO training (row a14: loss.backward() of main_simulation_simple_no.py:267-280) ---- */

/* Gradient outputs of ONE layer, same tensors and shapes as nonode_layer_weights (written, not
 * accumulated). */
typedef struct {
  float* edge_w1; float* edge_b1;
  float* edge_w2; float* edge_b2;
  float* coord_w1; float* coord_b1;
  float* coord_w2; float* coord_b2;
  float* vel_w1; float* vel_b1;
  float* vel_w2; float* vel_b2;
  float* node_w1; float* node_b1;
  float* node_w2; float* node_b2;
} nonode_layer_grads;

/* Floats in one backward blob (unscaled forward + transposed fragments). */
size_t nonode_bwd_blob_floats(void);
/* Pack one EGNO (or SEGNO) layer for the backward pass. */
int nonode_pack_layer_bwd(const nonode_layer_weights* w, int variant, int hidden, int n_edge_feat,
                          float* bblob, void* stream);
/* nonode_pack_layer_bwd of n_layers layers in one launch (w, bblobs: host arrays; same rules). */
int nonode_pack_layers_bwd(const nonode_layer_weights* const* w, int n_layers, int variant, int hidden,
                           int n_edge_feat, float* const* bblobs, void* stream);

/* Bytes of the saved forward state (every layer's inputs, message / force sums, embedding rows). */
size_t nonode_egno_train_state_bytes(int B, int N, int T, int n_layers, int in_node, int time_emb_dim);

/* EGNO.forward (egno.py:37-111) that also saves the state the backward needs. Same arguments and
 * outputs as nonode_egno_forward plus the state buffer. Outputs equal nonode_egno_forward's. */
int nonode_egno_forward_train(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                              int time_emb_dim, int modes, int Bt,
                              const float* x, const float* h, const float* v, const float* loc_mean,
                              const float* edge_fea, const float* t_out,
                              const float* emb_w, const float* emb_b,
                              const float* const* blobs, const float* const* tconv_blobs,
                              const float* const* tconvx_w,
                              float* x_out, float* v_out, float* h_out,
                              void* state, size_t state_bytes,
                              void* workspace, size_t workspace_bytes, void* stream);

size_t nonode_egno_backward_workspace_bytes(int B, int N, int T, int modes);

/* Reverse of nonode_egno_forward_train: given dL/dx_out (and optionally dL/dv_out, dL/dh_out;
 * NULL = 0), writes the gradient of every EGNO parameter: per layer (layer_grads[l]), the raw
 * TimeConv / TimeConv_x weights1 ([64][64][modes][2], [2][2][modes][2]) and the embedding Linear.
 * bblobs from nonode_pack_layer_bwd; tconv_w / tconvx_w are the raw weights1 tensors. */
int nonode_egno_backward(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                         int time_emb_dim, int modes, int Bt,
                         const float* loc_mean, const float* edge_fea,
                         const float* const* bblobs, const float* const* tconv_w,
                         const float* const* tconvx_w, const void* state,
                         const float* g_x, const float* g_v, const float* g_h,
                         const nonode_layer_grads* layer_grads, float* const* g_tconv,
                         float* const* g_tconvx, float* g_emb_w, float* g_emb_b,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * Multi-input (num_inputs > 1) training: nonode_egno_forward_train / nonode_egno_backward with the
 * inputs per frame as in nonode_egno_forward_frames (x, h, v, loc_mean [T*B*N] rows, edge_fea
 * [T*B*N*(N-1)] rows, t_in [Bt][T]). The state is sized by nonode_egno_train_state_bytes with
 * time_emb_dim doubled when t_in is given; backward takes with_t_in to match.
 */
int nonode_egno_forward_train_frames(int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                                     int time_emb_dim, int modes, int Bt, const float* x, const float* h,
                                     const float* v, const float* loc_mean, const float* edge_fea,
                                     const float* t_in, const float* t_out, const float* emb_w, const float* emb_b,
                                     const float* const* blobs, const float* const* tconv_blobs,
                                     const float* const* tconvx_w, float* x_out, float* v_out, float* h_out,
                                     void* state, size_t state_bytes, void* workspace, size_t workspace_bytes,
                                     void* stream);
int nonode_egno_backward_frames(int B, int N, int T, int n_layers, int in_node, int n_edge_feat, int time_emb_dim,
                                int with_t_in, int modes, int Bt, const float* loc_mean, const float* edge_fea,
                                const float* const* bblobs, const float* const* tconv_w,
                                const float* const* tconvx_w, const void* state, const float* g_x, const float* g_v,
                                const float* g_h, const nonode_layer_grads* layer_grads, float* const* g_tconv,
                                float* const* g_tconvx, float* g_emb_w, float* g_emb_b, void* workspace,
                                size_t workspace_bytes, void* stream);

/*
 * Input gradients of EGNO.forward (egno.py:37-111: x.repeat / v.repeat :89-96, the embedding Linear
 * :63-76, x - loc_mean ... + loc_mean :103-107). Frame t of the forward read input slot
 * frame_input[t] (host array [T]; NULL = every frame reads slot 0, which n_inputs == 1 requires; the
 * multi-input model's repeat_elements_to_exact_shape map otherwise). Device outputs, each may be NULL
 * (not computed), written not accumulated, sums over the frames of a slot in frame order:
 * g_x_in, g_v_in, g_loc_mean [n_inputs][B*N][3], g_h_in [n_inputs][B*N][in_node]. g_h_in needs emb_w
 * (the embedding weight [64][in_node + time-embedding columns] the forward used); g_loc_mean needs
 * time convolutions (without them the forward does not read loc_mean).
 */
typedef struct {
  int n_inputs;
  const int* frame_input;
  const float* emb_w;
  float* g_x_in;
  float* g_v_in;
  float* g_h_in;
  float* g_loc_mean;
} nonode_input_grads;

/* nonode_egno_backward (frames = 0; with_t_in ignored) or nonode_egno_backward_frames (frames = 1)
 * that also writes the input gradients *inputs asks for. Same workspace size. With inputs NULL or all
 * four of its outputs NULL it issues exactly the launches of those two entries. */
int nonode_egno_backward_inputs(int frames, int B, int N, int T, int n_layers, int in_node, int n_edge_feat,
                                int time_emb_dim, int with_t_in, int modes, int Bt, const float* loc_mean,
                                const float* edge_fea, const float* const* bblobs, const float* const* tconv_w,
                                const float* const* tconvx_w, const void* state, const float* g_x, const float* g_v,
                                const float* g_h, const nonode_layer_grads* layer_grads, float* const* g_tconv,
                                float* const* g_tconvx, float* g_emb_w, float* g_emb_b, void* workspace,
                                size_t workspace_bytes, void* stream, const nonode_input_grads* inputs);

/*
 * SEGNO training (replaces loss.backward() of SEGNO/train_nbody.py:168-179 through forward_step,
 * SEGNO/models/model.py:95-102, = T applications of SEGNO_GCL.forward, gcl.py:111-119, dt = 1/T).
 * nonode_segno_forward_train: forward_step from an embedded h [B*N][64] (the caller's embedding
 * Linear, model.py:73, stays on the autograd tape) that also saves every substep's inputs and sums;
 * outputs equal nonode_segno_forward_step's. blob: nonode_pack_layer(..., NONODE_VARIANT_SEGNO, ...).
 * nonode_segno_backward: given the gradients of (x, v, h) after the T substeps (g_v, g_h may be
 * null = zero), writes the gradients of the shared GCL weights into *grads (vel_* fields unused:
 * coord_mlp_vel is not on SEGNO's forward path) and of the inputs h, x, v (each may be null).
 * bblob: nonode_pack_layer_bwd(..., NONODE_VARIANT_SEGNO, ...).
 */
size_t nonode_segno_train_state_bytes(int B, int N, int T);
int nonode_segno_forward_train(int B, int N, int T, int n_edge_feat, const float* h, const float* x,
                               const float* v, const float* edge_attr, const float* blob, float coords_weight,
                               int recurrent, float* x_out, float* v_out, float* h_out, void* state,
                               size_t state_bytes, void* stream);
size_t nonode_segno_backward_workspace_bytes(int B, int N);
int nonode_segno_backward(int B, int N, int T, int n_edge_feat, float coords_weight, int recurrent,
                          const float* edge_attr, const float* bblob, const void* state, const float* g_x,
                          const float* g_v, const float* g_h, const nonode_layer_grads* grads, float* g_h_in,
                          float* g_x_in, float* g_v_in, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The embedding Linear of SEGNO (SEGNO/models/model.py:73, h = embedding(his), 64 outputs) as a
 * forward / backward pair, for a training caller that keeps it off the autograd tape:
 * nonode_embedding_forward: out[n][o] = bias[o] + sum_k weight[o][k] in[n][k] (in_features <= 40);
 * nonode_embedding_backward: grad_weight [64][in_features] = sum_n grad_out[n] (x) in[n], grad_bias =
 * sum_n grad_out[n] (written; a fixed summation order: deterministic).
 */
int nonode_embedding_forward(int n_rows, int in_features, const float* in, const float* weight, const float* bias,
                             float* out, void* stream);
size_t nonode_embedding_backward_workspace_bytes(int n_rows, int in_features);
int nonode_embedding_backward(int n_rows, int in_features, const float* in, const float* grad_out,
                              float* grad_weight, float* grad_bias, void* workspace, size_t workspace_bytes,
                              void* stream);

/*
 * Layer-granular reverse passes (SURVEY §8(b) egno_layer_bwd / spectral_tconv_bwd): autograd of ONE
 * EGNN_Layer or ONE TimeConv + TimeConv_x given that block's inputs and the gradients of its outputs,
 * for a caller that differentiates the blocks separately. Each recomputes what it needs of its forward
 * (message / force sums, LeakyReLU decisions) into the workspace; the whole-model
 * nonode_egno_backward runs the same reverse kernels from its saved state instead.
 *
 * nonode_egnn_layer_bwd: EGNN_Layer.forward (basic.py:167-186; variant NONODE_VARIANT_EGNO) over
 * n_graphs fully connected graphs of N nodes (N <= 115: the edge backward's LDS tables; a larger N
 * returns NONODE_EUNSUPPORTED before any launch; edge features of graph g from sample
 * g % ef_mod) with inputs h [n][64], x, v [n][3] (n = n_graphs N). blob / bblob from
 * nonode_pack_layer / nonode_pack_layer_bwd. Given dL/dx_out (g_v, g_h: NULL = 0) writes every
 * parameter gradient of the layer (*grads, written not accumulated) and dL/dh, dL/dx, dL/dv of the
 * inputs (dL/dv includes the output v, which the layer passes through unchanged).
 */
size_t nonode_egnn_layer_bwd_workspace_bytes(int n_graphs, int N);
int nonode_egnn_layer_bwd(int variant, int n_graphs, int N, int n_edge_feat, int ef_mod, const float* h,
                          const float* x, const float* v, const float* edge_fea, const float* blob,
                          const float* bblob, const float* g_x, const float* g_v, const float* g_h,
                          const nonode_layer_grads* grads, float* g_h_in, float* g_x_in, float* g_v_in,
                          void* workspace, size_t workspace_bytes, void* stream);
/*
 * nonode_egno_tconv_bwd: TimeConv + TimeConv_x of one EGNO layer (layer_no.py:80-178, egno.py:99-108)
 * on time-major [T][BN] inputs h [..][64], x, v [..][3] with loc_mean [BN][3], as nonode_egno_tconv
 * runs it (tconv_blob from nonode_pack_tconv; tconv_w / tconvx_w the raw weights1 tensors
 * [64][64][modes][2] / [2][2][modes][2], modes <= 9). Given the gradients of its outputs (NULL = 0)
 * writes the input gradients and the weights1 gradients.
 */
size_t nonode_egno_tconv_bwd_workspace_bytes(int BN, int T, int modes);
int nonode_egno_tconv_bwd(int BN, int T, int modes, const float* h, const float* x, const float* v,
                          const float* loc_mean, const float* tconv_blob, const float* tconv_w,
                          const float* tconvx_w, const float* g_h, const float* g_x, const float* g_v,
                          float* g_h_in, float* g_x_in, float* g_v_in, float* g_tconv_w, float* g_tconvx_w,
                          void* workspace, size_t workspace_bytes, void* stream);


/* ---- rollout drivers (rollout_fn / prepare_inputs / energy on the GPU) ---- */

/* prepare_inputs (EGNO/main_simulation_simple_no.py:311-339, num_inputs == 1) for B fully connected
 * graphs of N nodes, from frame f_b of F frames: loc, vel [F][B*N][3]; f_b = (t_in[b] - 1) mod F
 * (the reference's loc_all[timesteps_in.T - 1], python indexing) or the last frame if t_in is NULL.
 * Writes x_out, v_out [B*N][3], nodes [B*N][1 + (charges != NULL)] = [|v|, q],
 * edge_attr [B*N*(N-1)][n_eo + 1] = [edge_attr_o, |x_i - x_j|^2] (reference edge order), and
 * loc_mean [B*N][3] (per-graph mean; may be NULL). SEGNO's re-featurisation
 * (SEGNO/train_nbody.py:222-234) is the same call with charges = NULL, loc_mean = NULL. */
int nonode_prepare_inputs(int B, int N, int F, const float* loc, const float* vel, const int* t_in,
                          const float* charges, const float* edge_attr_o, int n_eo, float* x_out,
                          float* v_out, float* nodes, float* edge_attr, float* loc_mean, void* stream);

/* Reverse of nonode_prepare_inputs for what the reference keeps on the autograd tape (x_out, v_out and
 * loc_mean; nodes and edge_attr are detached, main_simulation_simple_no.py:321-338). Given g_x, g_v,
 * g_lm [B*N][3] (each may be NULL = 0) writes g_loc, g_vel [F][B*N][3] (each may be NULL):
 * g_loc[f_b][b][n] = g_x[b][n] + (1/N) sum_m g_lm[b][m], g_vel[f_b][b][n] = g_v[b][n], zero in every
 * other frame (f_b as in nonode_prepare_inputs). */
int nonode_prepare_inputs_bwd(int B, int N, int F, const int* t_in, const float* g_x, const float* g_v,
                              const float* g_lm, float* g_loc, float* g_vel, void* stream);

/* conserved_energy_fun (utils.py:197-219) of F frames x B graphs: loc, vel [F][B*N][3], weights [B*N]
 * (charges for kind 0 = charged, tot_energy_charged_batch utils.py:126-144; masses for kind 1 =
 * gravity, tot_energy_gravity_batch utils.py:175-195). out [F][B]. */
int nonode_energy(int kind, int F, int B, int N, const float* loc, const float* vel, const float* weights,
                  float* out, void* stream);

/* nonode_prepare_inputs_bwd for G graphs of mixed sizes (graph_ptr [G + 1], the exclusive prefix sum of the
 * sizes N_g >= 1 over n_total rows; t_in [G] or NULL): g_x, g_v, g_lm [n_total][3] -> g_loc, g_vel
 * [F][n_total][3], g_loc[f_g][n] = g_x[n] + (1/N_g) sum_m g_lm[m] over the rows m of n's graph, added in
 * node order (deterministic), zero in every other frame. */
int nonode_prepare_inputs_bwd_ragged(int G, int n_total, int F, const int* graph_ptr, const int* t_in,
                                     const float* g_x, const float* g_v, const float* g_lm, float* g_loc,
                                     float* g_vel, void* stream);

/* nonode_energy of F frames x G graphs of mixed sizes (graph_ptr as above): loc, vel [F][n_total][3], weights
 * [n_total], each energy over the graph's own nodes. out [F][G]. */
int nonode_energy_ragged(int kind, int F, int G, int n_total, const int* graph_ptr, const float* loc, const float* vel,
                         const float* weights, float* out, void* stream);

size_t nonode_egno_rollout_workspace_bytes(int B, int N, int T, int Bt, int in_node, int n_edge_feat);

/* rollout_fn (EGNO/main_simulation_simple_no.py:342-384, num_inputs == 1): traj_len segments of
 * nonode_egno_forward, each restarted from frame t_in[b]-1 (NULL: the last) through
 * nonode_prepare_inputs. x, h, v, loc_mean, edge_fea: segment-0 inputs (prepared by the caller);
 * t_out_all [Bt][traj_len*T] (segment i uses columns i*T.. minus i*T, :361-362); charges
 * [B*N] or NULL (nodes = [|v|(, q)] so in_node = 1 + (charges != NULL)); edge_attr_o [E][n_eo]
 * (n_edge_feat = n_eo + 1). Outputs loc_preds [traj_len*T][B*N][3]; energies (NULL = skip)
 * [traj_len*T][B] of every predicted frame with energy_kind / energy_w as in nonode_energy
 * (the reference's energies_allsteps; its per-segment `energies` are frames T-1, 2T-1, ...). */
int nonode_egno_rollout(int B, int N, int T, int n_layers, int in_node, int n_edge_feat, int time_emb_dim,
                        int modes, int Bt, int traj_len, const float* x, const float* h, const float* v,
                        const float* loc_mean, const float* edge_fea, const float* t_out_all, const int* t_in,
                        const float* charges, const float* edge_attr_o, int n_eo, int energy_kind,
                        const float* energy_w, const float* emb_w, const float* emb_b,
                        const float* const* blobs, const float* const* tconv_blobs,
                        const float* const* tconvx_w, float* loc_preds, float* energies,
                        void* workspace, size_t workspace_bytes, void* stream);

size_t nonode_segno_rollout_workspace_bytes(int B, int N, int in_node, int n_edge_feat);

/* rollout_fn (SEGNO/train_nbody.py:200-236, num_prev == 1): segment i runs SEGNO.forward with
 * substeps[i] (host array; the list form of num_steps, :209-212) integrator substeps, then
 * re-featurises h = |v|, edge_attr = [edge_attr_o, |x_i - x_j|^2]. his, x, v, edge_attr: segment-0
 * inputs. Outputs loc_preds [traj_len][B*N][3], energies [traj_len][B] (NULL = skip). */
int nonode_segno_rollout(int B, int N, int in_node, int n_edge_feat, int traj_len, const int* substeps,
                         const float* his, const float* x, const float* v, const float* edge_attr,
                         const float* edge_attr_o, int n_eo, int energy_kind, const float* energy_w,
                         const float* emb_w, const float* emb_b, const float* blob, float coords_weight,
                         int recurrent, float* loc_preds, float* energies, void* workspace,
                         size_t workspace_bytes, void* stream);


/* ---- synthetic N-body data (synthetic_sim.py on the GPU, float64) ---- */

/* ChargedParticlesSim.sample_trajectory (synthetic_sim.py:220-296) for S trajectories in one launch:
 * loc0, vel0 [S][3][N] the initial state after the reference's velocity normalisation and wall
 * clamp; charges [S][N]; Coulomb forces strength q_i q_j (x_i - x_j) / |x_i - x_j|^3 clamped to
 * +-max_F per component; leapfrog with step dt. Outputs loc_out, vel_out [S][T/sample_freq - 1][3][N]
 * (the reference's samples at steps sample_freq, 2 sample_freq, ...). N <= 1024 (one workgroup holds a
 * trajectory); nonode_sim_charged_tiled takes larger N. */
int nonode_sim_charged(int S, int N, int T, int sample_freq, double dt, double max_F, double strength,
                       const double* loc0, const double* vel0, const double* charges, double* loc_out,
                       double* vel_out, void* stream);

/* GravitySim.sample_trajectory_batch (synthetic_sim.py:407-481): pos0, vel0 [S][N][3] (centre-of-mass
 * velocity already removed), mass [S][N]; softened gravity, kick-drift-kick with step dt. Outputs
 * pos_out, vel_out, force_out (= a m) [S][T/sample_freq][N][3] sampled at steps 0, sample_freq, ...
 * N <= 1024 (one workgroup holds a trajectory); nonode_sim_gravity_tiled takes larger N. */
int nonode_sim_gravity(int S, int N, int T, int sample_freq, double dt, double G, double softening,
                       const double* pos0, const double* vel0, const double* mass, double* pos_out,
                       double* vel_out, double* force_out, void* stream);

/* The tiled simulators: the same trajectories for any N up to 2^20 with S N < 2^31, one launch per time
 * step (a workgroup owns a tile of receivers and stages the trajectory's senders through LDS in chunks;
 * every force sum runs over j = 0 .. N-1 in ascending order, so at N <= 1024 the outputs equal the
 * entries' above bit for bit). nonode_sim_tiled_shape reports the tile: receivers per workgroup and
 * senders per LDS chunk. */
int nonode_sim_tiled_shape(int* receivers, int* senders);

/* Bytes of workspace for the two entries below: 9 S N doubles (two position buffers [3][S N] and the
 * velocities [S N][3]). Host only; 0 for sizes the entries refuse (S < 1, N < 1, N > 2^20, S N >= 2^31). */
size_t nonode_sim_tiled_workspace_bytes(int S, int N);

/* GravitySim.sample_trajectory_batch (synthetic_sim.py:407-481) as nonode_sim_gravity computes it, same
 * layouts and sampling; N in [1, 2^20]. workspace: device memory, 8-byte aligned, at least
 * nonode_sim_tiled_workspace_bytes(S, N). Bad sizes, T % sample_freq != 0, a null pointer or a short
 * workspace return NONODE_EINVAL before any device work. */
int nonode_sim_gravity_tiled(int S, int N, int T, int sample_freq, double dt, double G, double softening,
                             const double* pos0, const double* vel0, const double* mass, double* pos_out,
                             double* vel_out, double* force_out, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ChargedParticlesSim.sample_trajectory (synthetic_sim.py:220-296) as nonode_sim_charged computes it, same
 * layouts and sampling; N in [2, 2^20]. workspace and refusals as nonode_sim_gravity_tiled. */
int nonode_sim_charged_tiled(int S, int N, int T, int sample_freq, double dt, double max_F, double strength,
                             const double* loc0, const double* vel0, const double* charges, double* loc_out,
                             double* vel_out, void* workspace, size_t workspace_bytes, void* stream);


/* ---- dataset -> device batches ---- */

/* One batch of NBodyDynamicsDataset (EGNO/simulation/dataset_simple.py:122-178) gathered from a
 * split resident on the device: loc, vel [S][Tf][N][3] (the .npy trajectories in
 * [sample][frame][node][xyz] order), charges [S][N], edge_attr_src [S][N*(N-1)] (the loader's q_i q_j
 * in the reference edge order, dataset_simple.py:46-72); batch row b is sample idx[b] with the I
 * input frames frame0[b][0..I) (num_inputs, dataset_simple.py:133-148; I = 1 for a single input) and
 * target frames out_idx[b][0..To). Writes loc0, vel0 [B][I][N][3], charges_out [B][N],
 * edge_attr [B][N*(N-1)] and loc_true [B][N][To][3] (locs_out). Index arrays are device int32 and
 * must be in range (the Python loader checks them). */
int nonode_gather_batch(int S, int Tf, int N, int B, int I, int To, const float* loc, const float* vel,
                        const float* charges, const float* edge_attr_src, const int* idx, const int* frame0, const int* out_idx,
                        float* loc0, float* vel0, float* charges_out, float* edge_attr, float* loc_true,
                        void* stream);

/* dst[b][0..K) = src[idx[b]][0..K) for b < B: whole samples of a device-resident split
 * (SEGNO/dataset_nbody.py:82-86 __getitem__ + default_collate; one launch per array). src, dst
 * 16-byte aligned; idx device int32 in [0, S). */
int nonode_gather_rows(int S, long long K, int B, const float* src, const int* idx, float* dst, void* stream);

/* ---- EGNO(flat=True) training (main_simulation_simple_no.py --flat; basic.py:38-40) ---- */

/* One flat EGNN layer forward (EGNN_Layer.forward, basic.py:167-186, every BaseMLP 256 wide with
 * Tanh) that keeps its state for the reverse pass: state [nonode_egnn_layer_flat_state_floats] holds
 * the per-node projections P, Q [n][256], message sums M [n][64] and force sums F [n][4]. */
size_t nonode_egnn_layer_flat_state_floats(int n_graphs, int N);
int nonode_egnn_layer_flat(int n_graphs, int N, int n_edge_feat, int ef_mod, const float* h, const float* x,
                           const float* v, const float* edge_fea, const float* blob, float* h_out, float* x_out,
                           float* state, void* stream);
/* Transposed fragments of a flat layer's 256-wide matrices for the reverse pass. */
size_t nonode_flat_bwd_blob_floats(void);
int nonode_pack_layer_flat_bwd(const nonode_layer_weights* w, int n_edge_feat, float* bblob, void* stream);
/* Reverse of nonode_egnn_layer_flat (autograd of basic.py:107-186 with flat=True) given the gradients of
 * its outputs: per node (node_ops [n][1676]: h part of dL/dh, dL/dM, dL/dF, dL/dx, the receiver / sender
 * sums GA, GB [256] of dL/d(first Linear output), and the node MLPs' activations and gradients) and per
 * edge (edge_ops [n (N-1)][1160]: the edge MLPs' activations and gradients, the scalar inputs) the operands of every
 * weight gradient (each one a GEMM over nodes or edges, the caller's), and dL/dv of the input. */
size_t nonode_egnn_layer_flat_bwd_node_floats(int n_graphs, int N);
size_t nonode_egnn_layer_flat_bwd_edge_floats(int n_graphs, int N);
int nonode_egnn_layer_flat_bwd(int n_graphs, int N, int n_edge_feat, int ef_mod, const float* h, const float* x,
                               const float* v, const float* edge_fea, const float* blob, const float* bblob,
                               const float* state, const float* g_x, const float* g_v, const float* g_h,
                               float* node_ops, float* edge_ops, float* g_v_in, void* stream);

/* ---- the fully connected edge list at the boundary (sync-free) ---- */

/* NBodyDataset.get_edges (EGNO/simulation/dataset_simple.py:101-111; SEGNO/dataset_nbody.py:84-94) on
 * the device: rows, cols [B*N*(N-1)] int64, receiver i, sender j != i, ordered by (sample, i, j). */
int nonode_full_edges(int B, int N, long long* rows, long long* cols, void* stream);

/* Validate the `edges` argument of EGNO.forward (egno.py:37) / SEGNO.forward (model.py:53) on the
 * device, without blocking the host: rows, cols (E indices of idx_bytes = 4 or 8 bytes) must be
 * exactly nonode_full_edges(B, N). Any mismatch sets the device int *flag to 1 (never to 0: the
 * caller clears it after reading it). */
int nonode_check_full_edges(const void* rows, const void* cols, int idx_bytes, long long E, int B, int N, int* flag,
                            void* stream);

/* If *flag is set when the launch runs, fill bufs[k][0..counts[k]) (k < n_bufs <= 4, fp32) with NaN:
 * the outputs of a forward whose edge list failed nonode_check_full_edges. */
int nonode_poison_if_flagged(const int* flag, int n_bufs, float* const* bufs, const long long* counts, void* stream);


/* ---- arbitrary edge lists: CSR graph kernels (inference, and the EGNO layer's reverse) ---- */

/*
 * The `edges` argument of EGNN_Layer.forward (basic.py:167-186, aggregate basic.py:6-31) and
 * SEGNO_GCL.forward (gcl.py:111-119, unsorted_segment_mean) as a CSR by receiver, built on the device:
 * rows (receivers), cols (senders): E indices of idx_bytes = 4 or 8 bytes, E < 2^31. Writes
 * row_ptr [n_nodes + 1], col [E], eid [E] (original edge index), all int32. Within a receiver the
 * edges are ordered by (sender, original index), so the CSR is a pure function of the edge set. Self
 * loops and duplicate edges are kept (the reference sums them). An index outside [0, n_nodes) sets the
 * device int *flag to 1 (never to 0) and that edge is dropped: row_ptr[n_nodes] counts the kept edges,
 * and nothing downstream reads an index that was not range-checked. E = 0 is legal.
 * Workspace: nonode_graph_workspace_bytes(E, n_nodes).
 */
size_t nonode_graph_workspace_bytes(long long E, int n_nodes);
int nonode_graph_build(const void* rows, const void* cols, int idx_bytes, long long E, int n_nodes, int* row_ptr,
                       int* col, int* eid, int* flag, void* workspace, size_t workspace_bytes, void* stream);

/*
 * nonode_egnn_layer on an explicit edge list: EGNN_Layer.forward (basic.py:167-186) for variant EGNO,
 * SEGNO_GCL.forward (gcl.py:111-119) for variant SEGNO, over n_frames copies of one n_nodes-node graph
 * given as the CSR of nonode_graph_build. Frame f owns node rows f*n_nodes .. of h [.][64], x, v [.][3]
 * (EGNO's T-fold replication, egno.py:84-96); its edge features are block f % ef_frames of edge_fea
 * [ef_frames][E][n_edge_feat], read at eid. blob from nonode_pack_layer (its NORM_RADIAL / TANH_COORD
 * flags are followed). A node without incoming edges gets zero message and force sums and the mean's
 * count.clamp(min=1) (basic.py:28, gcl.py unsorted_segment_mean). dt, coords_weight, recurrent, v_out
 * as nonode_egnn_layer. Per-receiver sums are added in CSR order without float atomics: bitwise
 * reproducible. Workspace: nonode_egnn_layer_graph_workspace_bytes(n_frames, n_nodes).
 */
size_t nonode_egnn_layer_graph_workspace_bytes(int n_frames, int n_nodes);
int nonode_egnn_layer_graph(int variant, int n_frames, int n_nodes, long long E, int n_edge_feat, int ef_frames,
                            const float* h, const float* x, const float* v, const float* edge_fea, const float* blob,
                            const int* row_ptr, const int* col, const int* eid, float dt, float coords_weight,
                            int recurrent, float* h_out, float* x_out, float* v_out, void* workspace,
                            size_t workspace_bytes, void* stream);

/*
 * ---- training on an explicit edge list (EGNO graph="trainable"; csrc/nonode_graph_train.hip) ----
 *
 * The training forward of the graph layer IS nonode_egnn_layer_graph: its workspace is the state the
 * reverse pass reads, so a caller that trains keeps the workspace alive until the backward. Layout
 * (floats, n = n_frames * n_nodes): P [n][64] | Q [n][64] (the first edge Linear's receiver / sender
 * projections, InvariantScalarNet basic.py:107-123, in the packed blob's log2-domain scale), M [n][64]
 * (message sums, aggregate basic.py:6-31, same scale), F [n][4] = (force sum x3, in-degree).
 *
 * nonode_graph_edge_mask: valid[e] = 1 for every edge nonode_graph_build kept (row_ptr, eid of the CSR
 * by receiver), 0 for the ones it dropped (an index out of range).
 *
 * nonode_egnn_layer_graph_bwd, variant EGNO: the reverse of EGNN_Layer.forward (basic.py:167-186:
 * edge message basic.py:170 / 107-144, coord_net and the aggregate basic.py:171-177 / 6-31, node_v_net
 * and the x update basic.py:178-181, node_net basic.py:182-185) for frames [f0, f1) of the n_frames the
 * forward ran. Inputs: the layer's inputs h, x, v, edge_fea, its forward blob, the backward blob of
 * nonode_pack_layer_bwd, the forward's state, the CSR by receiver (row_ptr, col, eid), the CSR by sender
 * (srow_ptr, seid: nonode_graph_build with rows and cols swapped), valid (nonode_graph_edge_mask, or
 * NULL when no edge was dropped) and the gradients g_x, g_v, g_h of x_out, v_out, h_out (full
 * [n_frames * n_nodes] arrays; NULL = 0). Writes rows f0 * n_nodes .. f1 * n_nodes of g_h_in [.][64],
 * g_x_in, g_v_in [.][3], and the operands of the weight gradients for those frames, rows relative to f0:
 *   node_ops [(f1-f0) n_nodes][520]: 0 dL/dh part | 64 dL/dM | 128 gz (node_net hidden pre-activation
 *     gradient) | 192 z (its activation) | 256 gt | 320 t (node_v_net likewise) | 384 GA = sum over
 *     incoming edges of gz1 | 448 GB = sum over outgoing edges of gz1 | 512 dL/dF x3, gphi | 516 the
 *     receiver's share of dL/dx x3, 0
 *   edge_ops [(f1-f0)][E][400], row = the edge's ORIGINAL index: 0 gz1 | 64 gz2 | 128 a | 192 (1, s, e_0 ..
 *     e_3, 0, 0: the ones column, the radial input, the edge's features) | 200 gz3 | 264 gc, dL/dr x3 |
 *     268 m | 332 (1, 0, 0, 0) | 336 c1 (gz*: the edge MLP's and coord_net's pre-activation gradients; a, m,
 *     c1: their true-scale activations). Rows of dropped edges are zero when valid is given.
 * Every weight gradient is a sum over nodes or edges of outer products of these rows (the caller's GEMMs,
 * accumulated over frame groups; the edge-level ones are [gz1 | gz2]^T [a | 1, s, e] and
 * [gz3 | gc]^T [m | 1 | c1]): the frame range bounds edge_ops. No float atomics: per-receiver and
 * per-sender sums are added in CSR order, so g_*_in are bitwise reproducible and, for a list without
 * duplicate edges, independent of the list's order. Asynchronous; allocates nothing.
 */
int nonode_graph_edge_mask(const int* row_ptr, const int* eid, int n_nodes, long long E, int* valid, void* stream);
size_t nonode_egnn_layer_graph_bwd_node_floats(int n_frames, int n_nodes);
size_t nonode_egnn_layer_graph_bwd_edge_floats(int n_frames, long long E);
int nonode_egnn_layer_graph_bwd(int variant, int n_frames, int n_nodes, long long E, int n_edge_feat, int ef_frames,
                                int f0, int f1, const float* h, const float* x, const float* v, const float* edge_fea,
                                const float* blob, const float* bblob, const float* state, const int* row_ptr,
                                const int* col, const int* eid, const int* srow_ptr, const int* seid, const int* valid,
                                const float* g_x, const float* g_v, const float* g_h, float* node_ops, float* edge_ops,
                                float* g_h_in, float* g_x_in, float* g_v_in, void* stream);

/*
 * EGNO.forward (EGNO/model/egno.py:37-111) on an explicit edge list: the arguments of
 * nonode_egno_forward_flat with (B, N) replaced by n_nodes, E and the CSR, and blobs from
 * nonode_pack_layer. t_in = NULL: the single-input layout of nonode_egno_forward (x, v, loc_mean
 * [n_nodes][3], h [n_nodes][in_node], edge_fea [E][n_edge_feat]); otherwise the per-frame layout of
 * nonode_egno_forward_frames ([T*n_nodes] rows, edge_fea [T][E][n_edge_feat]). tconv_blobs = tconvx_w
 * = NULL: use_time_conv=False. Outputs [T*n_nodes] rows, time-major. n_nodes % Bt == 0.
 * Workspace: nonode_egno_graph_workspace_bytes(n_nodes, T, Bt).
 */
size_t nonode_egno_graph_workspace_bytes(int n_nodes, int T, int Bt);
int nonode_egno_forward_graph(int n_nodes, long long E, int T, int n_layers, int in_node, int n_edge_feat,
                              int time_emb_dim, int modes, int Bt, const float* x, const float* h, const float* v,
                              const float* loc_mean, const float* edge_fea, const float* t_in, const float* t_out,
                              const float* emb_w, const float* emb_b, const float* const* blobs,
                              const float* const* tconv_blobs, const float* const* tconvx_w, const int* row_ptr,
                              const int* col, const int* eid, float* x_out, float* v_out, float* h_out,
                              void* workspace, size_t workspace_bytes, void* stream);

/*
 * SEGNO.embedding + SEGNO.forward_step (SEGNO/models/model.py:73,95-102) on an explicit edge list: the
 * arguments of nonode_segno_forward_step with (B, N) replaced by n_nodes, E and the CSR; edge_attr
 * [E][n_edge_feat] is frozen over the T substeps. Workspace: nonode_segno_graph_workspace_bytes(n_nodes).
 */
size_t nonode_segno_graph_workspace_bytes(int n_nodes);
int nonode_segno_forward_step_graph(int n_nodes, long long E, int T, int in_node, int n_edge_feat, const float* his,
                                    const float* h_in, const float* x, const float* v, const float* edge_attr,
                                    const float* emb_w, const float* emb_b, const float* blob, const int* row_ptr,
                                    const int* col, const int* eid, float coords_weight, int recurrent, float* x_out,
                                    float* v_out, float* h_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ---- SEGNO training on an explicit edge list (SEGNO graph="any", trainable=True) ----
 *
 * nonode_segno_forward_train_graph: SEGNO.forward_step (SEGNO/models/model.py:95-102) from an embedded h
 * [n_nodes][64] on the tape, as T calls of the graph layer (SEGNO_GCL.forward, gcl.py:111-119, dt = 1/T,
 * edge_attr [E][n_edge_feat] frozen). Outputs are bitwise those of nonode_segno_forward_step_graph with
 * h_in = h. It keeps every substep's inputs and its layer workspace in `state`
 * (nonode_segno_graph_train_state_bytes(n_nodes, T) = T * n_nodes * 266 floats; n = n_nodes):
 *   hs [T][n][64] | ws [T][n * 196] | xs [T][n][3] | vs [T][n][3]
 * hs[t], xs[t], vs[t]: the inputs of substep t (index 0: copies of h, x, v); ws[t]: that substep's
 * P [n][64] | Q [n][64] | M [n][64] | F [n][4], the state layout of nonode_egnn_layer_graph above. The
 * caller keeps `state` alive until the backward. T = 0 copies the inputs through (state may be NULL);
 * E = 0 is legal. Asynchronous; allocates nothing.
 *
 * nonode_segno_layer_graph_bwd: the reverse of ONE substep, SEGNO_GCL.forward (gcl.py:111-119: edge_model
 * gcl.py:74-83, coord_model's per-edge clamp and segment mean gcl.py:97-102 / 16-24, node_model gcl.py:85-95,
 * v' = v + coords_weight mean dt, x' = x + v' dt) on the CSRs. Arguments as nonode_egnn_layer_graph_bwd
 * with n_frames = 1 (h, x, v: the substep's inputs hs[t], xs[t], vs[t]; state: ws[t]; bblob from
 * nonode_pack_layer_bwd, variant SEGNO), plus dt, coords_weight, recurrent. node_ops [n_nodes][520] and
 * edge_ops [E][400] keep the layout above, so the caller's weight-gradient GEMMs are shared; the gt, t and
 * gphi slots (256, 320, 515) carry nothing: the first two are not written and gphi is 0. The edge MLP's
 * first Linear has input order [h_i, h_j, s, e] (gcl.py:78): its gradient's columns are GA^T h | GB^T h |
 * gz1^T s | gz1^T e. The clamp passes dL/dF per edge and component where -100 <= r_k c <= 100. No float
 * atomics, sums in CSR order, rows of dropped edges zero when valid is given; NONODE_EUNSUPPORTED /
 * NONODE_EINVAL before any launch.
 */
size_t nonode_segno_graph_train_state_bytes(int n_nodes, int T);
int nonode_segno_forward_train_graph(int n_nodes, long long E, int T, int n_edge_feat, const float* h, const float* x,
                                     const float* v, const float* edge_attr, const float* blob, const int* row_ptr,
                                     const int* col, const int* eid, float coords_weight, int recurrent, float* x_out,
                                     float* v_out, float* h_out, void* state, size_t state_bytes, void* stream);
int nonode_segno_layer_graph_bwd(int n_nodes, long long E, int n_edge_feat, const float* h, const float* x,
                                 const float* v, const float* edge_attr, const float* blob, const float* bblob,
                                 const float* state, const int* row_ptr, const int* col, const int* eid,
                                 const int* srow_ptr, const int* seid, const int* valid, const float* g_x,
                                 const float* g_v, const float* g_h, float dt, float coords_weight, int recurrent,
                                 float* node_ops, float* edge_ops, float* g_h_in, float* g_x_in, float* g_v_in,
                                 void* stream);

/*
 * ---- neighbour graphs built on the device, featurisation on an explicit list (csrc/nonode_neighbor.hip) ----
 *
 * nonode_neighbor_graph stands in for no reference code: the reference builds only full graphs. It is
 * what a rollout on a k-NN / cut-off graph calls every segment (the drivers harness.egno_rollout_graph /
 * segno_rollout_graph mirror rollout_fn, main_simulation_simple_no.py:342-384 and train_nbody.py:200-236,
 * as loops of model segments over these entries). Training on such a graph (a taped EGNO forward, the
 * unrolled harness.egno_rollout_train_graph) also needs its CSR by sender: nonode_neighbor_by_sender below.
 *
 * The batch is B graphs of N consecutive rows of x [B*N][3]. A candidate of receiver i is a node j != i of
 * the same graph with d2 <= r2_max true, where d = x_i - x_j componentwise and
 * d2 = ((d0*d0) + (d1*d1)) + (d2*d2), every operation rounded to f32 on its own (no fused multiply-add;
 * a NaN distance is never a candidate). Row i keeps the min(k, candidates) smallest candidates under the
 * total order (d2, j) and lists them by ascending sender: the CSR nonode_graph_build gives the same edge
 * set. With E = row_ptr[B*N] and cap = B*N*min(k, N-1): for p < E, col[p] = sender and rows[p] = receiver
 * (global row indices), eid[p] = p; for E <= p < cap, col[p] = rows[p] = -1, eid[p] = p. k in [1, 64];
 * r2_max > 0, +inf allowed. No float atomics, no launch sized from device data: bitwise reproducible.
 * Asynchronous. Workspace: nonode_neighbor_graph_workspace_bytes(B, N, k).
 */
size_t nonode_neighbor_graph_workspace_bytes(int B, int N, int k);
int nonode_neighbor_graph(int B, int N, int k, float r2_max, const float* x, int* row_ptr, int* col, int* eid,
                          int* rows, void* workspace, size_t workspace_bytes, void* stream);

/*
 * nonode_neighbor_graph for a batch of G graphs of mixed sizes over the n_total rows of x [n_total][3]:
 * graph g is rows graph_ptr[g] .. graph_ptr[g + 1] (graph_ptr [G + 1], the exclusive prefix sum of the
 * sizes N_g >= 1, graph_ptr[G] = n_total), graph_of [n_total] names every row's graph, n_max is the largest
 * N_g (device pointers; the same kernels, which take a graph's bounds from here instead of from a division).
 * The contract above holds per graph: receiver r of graph g keeps the min(k, N_g - 1, candidates) nodes
 * j != r of its own graph with the smallest (d2, j), d2 and the candidates as above, listed by ascending
 * sender; a graph of one node has rows of degree 0. cap = sum_g N_g min(k, N_g - 1) (the caller's: the host
 * knows the sizes) is the length of col, rows, eid, with the (-1, -1, p) tail from E = row_ptr[n_total] up
 * to cap. A pure function of the positions and the sizes, bitwise; equal sizes give nonode_neighbor_graph's
 * arrays. Refused with NONODE_EINVAL before any launch: G < 1, n_total < G, n_total >= 2^30, n_max outside [1, n_total],
 * k outside [1, 64], r2_max not > 0, cap < 0, cap >= 2^31, cap > n_total*min(k, n_max - 1), null pointers.
 * A descriptor that disagrees with cap or n_total cannot make a kernel write outside [0, cap) of col, rows,
 * eid or [0, n_total] of row_ptr (graph bounds are held to [0, n_total], every store is guarded).
 * Asynchronous. Workspace: nonode_neighbor_graph_ragged_workspace_bytes(n_total, n_max, k) =
 * (n_total + n_total*min(k, n_max - 1)) ints (the rows at one fixed pitch); 0 for refused arguments.
 */
size_t nonode_neighbor_graph_ragged_workspace_bytes(int n_total, int n_max, int k);
int nonode_neighbor_graph_ragged(int G, int n_total, int n_max, int k, long long cap, float r2_max,
                                 const int* graph_ptr, const int* graph_of, const float* x, int* row_ptr, int* col,
                                 int* eid, int* rows, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same graph under a FINITE cut-off from a cell list instead of the search over all N_g nodes of a graph:
 * for every input, row_ptr, col, rows, eid and the (-1, -1, p) tail are bitwise what
 * nonode_neighbor_graph_ragged (nonode_neighbor_graph) writes; only the work differs, O(cells a cut-off box
 * touches) per receiver instead of O(N_g). Arguments as nonode_neighbor_graph_ragged; graph_ptr and graph_of
 * both NULL: G graphs of n_max rows each (n_total = G*n_max). Each graph's finite nodes are binned into a
 * uniform grid of g cells per axis, g the largest integer with 4 g^3 <= N_g, cell width max(rr, extent / g)
 * per axis, rr a search radius just above sqrt(r2_max) with rr*rr > r2_max in f32; the nodes are sorted by
 * cell and one wave per receiver walks the cells cell(x_i - rr) .. cell(x_i + rr) of every axis, feeding the
 * same distances and keys into the same keep-the-k-smallest code. One binning function, built from
 * individually rounded (hence monotone) f32 operations, bins the nodes and bounds the box, which is why no
 * candidate is missed whatever the rounding (csrc/nonode_cells.h). A node with a non-finite coordinate gets
 * degree 0 and is in no row, as the contract above implies under a finite r2_max. A stretched extent (one
 * outlier, a diverged rollout) leaves most nodes in few cells: the same graph, found more slowly.
 * Integer atomics count the cells and claim the sorted slots, so the order inside a cell varies from run to run;
 * the rows do not (the top k of a set under a total order). No launch, allocation or grid sized from device data.
 * Refused with NONODE_EINVAL: what nonode_neighbor_graph_ragged refuses, r2_max not finite, one of graph_ptr /
 * graph_of NULL and the other not, equal sizes with n_total != G*n_max, a workspace not 16-byte aligned.
 * Every store is guarded against a descriptor that disagrees with n_total or cap. Asynchronous.
 * Workspace: nonode_neighbor_graph_cells_workspace_bytes(G, n_total, n_max, k) =
 * (n_total*(8 + min(k, n_max - 1)) + 8 G + 1) ints (the sorted positions, the rows at one fixed pitch, the cell
 * table of n_total + G entries and its scan); 0 for refused arguments.
 */
size_t nonode_neighbor_graph_cells_workspace_bytes(int G, int n_total, int n_max, int k);
int nonode_neighbor_graph_cells(int G, int n_total, int n_max, int k, long long cap, float r2_max,
                                const int* graph_ptr, const int* graph_of, const float* x, int* row_ptr, int* col,
                                int* eid, int* rows, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Diagnostic, HOST arrays and no device: the grid, the binning and the search boxes of
 * nonode_neighbor_graph_cells, computed by the functions its kernels run. graph_ptr [G + 1] (NULL: G graphs
 * of n_max rows), x [n_total][3]. Outputs (each may be NULL): rr_out [1] the search radius; grid [G] the cells
 * per axis; box [G][9] = lower corner, upper corner, 1 / cell width per axis; cell [n_total][3] every node's
 * cell per axis (-1: a non-finite node has none); range [n_total][6] = the lowest and the highest cell per
 * axis that the node searches as a receiver (-1 for a non-finite node). Returns NONODE_OK or NONODE_EINVAL.
 */
int nonode_debug_neighbor_cells(int G, int n_total, int n_max, float r2_max, const int* graph_ptr, const float* x,
                                float* rr_out, int* grid, float* box, int* cell, int* range);

/*
 * The same graph for ANY r2_max > 0 (+inf: the pure k-NN graph) from the same cell list, the radius found per
 * receiver instead of being given: for every input, row_ptr, col, rows, eid and the (-1, -1, p) tail are bitwise
 * what nonode_neighbor_graph_ragged (nonode_neighbor_graph) writes. Arguments, refusals (all but the finiteness
 * of r2_max) and workspace as nonode_neighbor_graph_cells. The grid has cell width extent / g per axis. One wave
 * per receiver: (1) the box of cells [c - s, c + s] around its own cell c, s grown from 1 until the box holds
 * kk = min(k, N_g - 1) other nodes (from the cell table alone) or covers the grid, goes through the
 * keep-the-k-smallest code; D = the kk-th smallest d2 found, or r2_max if fewer were found and it is finite;
 * (2) the cut-off search with r2_max := D, a radius rr with rr*rr > D in f32 computed on the device, of which only
 * the cells outside the first box are still walked. Exact because the kk smallest keys all have d2 <= D (D is the
 * kk-th smallest over a subset) and every node with d2 <= D has its cell in the second box (the covering
 * argument of nonode_neighbor_graph_cells, csrc/nonode_cells.h). A receiver walks its whole graph instead (the
 * search of nonode_neighbor_graph on the sorted copy) when it has a non-finite coordinate, when kk = N_g - 1,
 * when D is not finite (under r2_max = +inf a node at +-inf is a candidate with d2 = inf, a NaN never is) or
 * when no rr is found. Bitwise reproducible, asynchronous, nothing sized from device data.
 */
size_t nonode_neighbor_graph_knn_cells_workspace_bytes(int G, int n_total, int n_max, int k);
int nonode_neighbor_graph_knn_cells(int G, int n_total, int n_max, int k, long long cap, float r2_max,
                                    const int* graph_ptr, const int* graph_of, const float* x, int* row_ptr, int* col,
                                    int* eid, int* rows, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Diagnostic, HOST arrays and no device: nonode_neighbor_graph_knn_cells receiver by receiver, through the
 * functions its kernel runs (the grid, the binning, the boxes, the radius, the distance and the keys), sequential
 * where the kernel is a wave. graph_ptr [G + 1] (NULL: G graphs of n_max rows), x [n_total][3]; k in [1, 64],
 * r2_max > 0 (+inf allowed). Outputs (each may be NULL), per receiver r: nbr [n_total][min(k, n_max - 1)] the kept
 * senders (global rows, ascending; -1 past the degree); deg [n_total]; d_out [n_total] the bound D (-1: phase 1
 * did not run); stats [n_total][16] = {the final half-width s of the first box (0: not run), its lowest cell per
 * axis [3], its highest [3], the second box likewise [3] [3] (-1: none), the number of distances evaluated, 1 if
 * the receiver walked its whole graph, the cells per axis g}. Returns NONODE_OK or NONODE_EINVAL.
 */
int nonode_debug_neighbor_knn_cells(int G, int n_total, int n_max, int k, float r2_max, const int* graph_ptr,
                                    const float* x, int* nbr, int* deg, int* stats, float* d_out);

/*
 * The same graph as a CSR by sender, which the reverse pass of the graph layer
 * (nonode_egnn_layer_graph_bwd) walks: what training on a graph rebuilt every step needs, made on the
 * device from the padded list and its device-side count (nonode_graph_build cannot take a list with a
 * -1 tail). With E = row_ptr[n_total], read on the device only (held to [0, cap]):
 *   srow_ptr [n_total + 1]  the exclusive scan of the out-degrees over the entries p < E
 *   seid [cap]              sender s's positions p < E with col[p] == s, ascending p, at
 *                           seid[srow_ptr[s] .. srow_ptr[s + 1]): the order (receiver, original index) of
 *                           nonode_graph_build with rows and cols swapped, as the list is receiver-major
 *                           and eid the identity; -1 at and past E
 *   valid [cap]             1 for p < E, 0 for the tail (the backward zeroes the edge_ops rows it marks 0)
 * No rows / col value at p >= E is used (rows is not read at all); a col[p] outside [0, n_total), which
 * nonode_neighbor_graph never writes, is skipped. Integer atomics count the out-degrees and claim slots;
 * a rank sort per sender (one wave per sender, a row of any length: a hub sends to up to N - 1 receivers,
 * not k) then puts each row in the total order above, so the result is bitwise the same from run to run.
 * No launch sized from device data. Asynchronous. cap == 0: srow_ptr all zero, nothing else touched.
 * Workspace: nonode_neighbor_by_sender_workspace_bytes(cap, n_total) (0 for cap < 0 or n_total <= 0).
 */
size_t nonode_neighbor_by_sender_workspace_bytes(long long cap, int n_total);
int nonode_neighbor_by_sender(long long cap, int n_total, const int* rows, const int* col, const int* row_ptr,
                              int* srow_ptr, int* seid, int* valid, void* workspace, size_t workspace_bytes,
                              void* stream);

/*
 * The node side of prepare_inputs (main_simulation_simple_no.py:311-339, num_inputs == 1) without its
 * full-graph edge column: loc, vel [F][B*N][3], frame t_in[b] - 1 of sample b (python index; NULL: the last
 * frame) -> x_out, v_out [B*N][3], nodes [B*N][1 + (charges != NULL)] = [|v|, q], loc_mean [B*N][3] (the
 * per-graph mean; NULL: skipped). Any N (nothing is staged per graph).
 */
int nonode_prepare_nodes(int B, int N, int F, const float* loc, const float* vel, const int* t_in,
                         const float* charges, float* x_out, float* v_out, float* nodes, float* loc_mean,
                         void* stream);

/*
 * nonode_prepare_nodes for G graphs of mixed sizes (graph_ptr [G + 1] as in nonode_neighbor_graph_ragged): loc,
 * vel [F][n_total][3], t_in [G] or NULL, charges [n_total] or NULL -> x_out, v_out, loc_mean [n_total][3],
 * nodes [n_total][1 + (charges != NULL)]. The mean is over the graph's own N_g rows, summed in a fixed tree
 * that depends on N_g alone: a graph of N rows gets bitwise the mean nonode_prepare_nodes gives it.
 */
int nonode_prepare_nodes_ragged(int G, int n_total, int F, const int* graph_ptr, const float* loc, const float* vel,
                                const int* t_in, const float* charges, float* x_out, float* v_out, float* nodes,
                                float* loc_mean, void* stream);

/*
 * The edge side on an explicit list (the reference computes these columns only in the full order:
 * main_simulation_simple_no.py:328-338, train_nbody.py:203,229-233): edge_attr[p] = [q_r*q_c, |x_r - x_c|^2]
 * ([cap][2]), or [|x_r - x_c|^2] ([cap][1]) with charges = NULL, for r = rows[p], c = cols[p] (idx_bytes 4
 * or 8) and p < *n_edges (a device pointer; NULL: p < cap). Rows at or past the count, and pairs with an
 * index outside [0, n_nodes), are zero. The distance uses nonode_neighbor_graph's arithmetic.
 */
int nonode_edge_features(long long cap, int n_nodes, const void* rows, const void* cols, int idx_bytes,
                         const int* n_edges, const float* x, const float* charges, float* edge_attr, void* stream);


/* ---- rollout metrics ---- */

/* Per (frame t, graph b) of pred, truth [T][B*N][3]: corr[b][t] = Pearson correlation over the
 * graph's N*3 coordinates (pearson_correlation_batch, utils.py:261-321) and sqerr[t][b] = summed
 * squared error (the per-horizon MSE of main_simulation_simple_no.py:273 is sum_b sqerr / (B*N*3)).
 * Either output may be NULL. */
int nonode_rollout_metrics(int T, int B, int N, const float* pred, const float* truth, float* corr,
                           float* sqerr, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NONODE_H_ */
