/*
 * grl.h -- C ABI of libgrl.so, the MI355X (gfx950) implementation of the SAC / DQN / BDQ
 * update hot path of BarisYazici/deep-rl-grasping.
 *
 * The reference has no FFI of its own: its hot path is the stable-baselines model object it
 * drives from Python.  Each entry point below names the reference call it stands behind
 * (paths relative to /root/reference):
 *
 *   grl_create / grl_destroy      sb.SAC(policy, env, policy_kwargs=..., gamma=..., buffer_size=...,
 *                                 batch_size=..., learning_rate=...)
 *                                 manipulation_main/training/sb_helper.py:104-112,120-128
 *   grl_param_count/info          model.get_parameters() / load_parameters()  sb_helper.py:114-115
 *   grl_replay_add                SAC.learn -> replay_buffer.add(obs, action, reward, new_obs, done)
 *                                 (stable-baselines learn loop entered at sb_helper.py:175-177)
 *   grl_set_obs_stats             VecNormalize(env, norm_obs=True, norm_reward=True, clip_obs=10.)
 *                                 statistics read at replay-sample time   sb_helper.py:117-119
 *   grl_train_step                SAC._train_step + target_update_op, once per env step
 *                                 (train_freq=1, gradient_steps=1)         sb_helper.py:175-177
 *   grl_compute_grads/apply_grads the same step split around the data-parallel gradient all-reduce
 *   grl_act                       model.predict(obs, deterministic)        manipulation_main/utils.py:71,
 *                                 training/base_callbacks.py:84-88
 *   grl_encode                    SimpleAutoEncoder.encode(imgs)           gripperEnv/encoders.py:59-61,
 *                                 call site gripperEnv/sensor.py:220-222
 *
 * Conventions
 *   - plain C types only; device memory is passed as raw pointers.  All device memory is OWNED BY
 *     THE CALLER (PyTorch-ROCm tensors in the Python host); the library allocates no device memory.
 *     Sizes of the arenas the caller must provide come from grl_query_sizes().
 *   - every call enqueues its work on the HIP stream given by grl_set_stream() (default: the null
 *     stream) and returns without synchronising, except the calls documented as "host" which copy
 *     results to host memory and synchronise that stream.
 *   - return value 0 = OK, negative = error; grl_last_error() returns a thread-local message.
 *   - one handle per GPU / process; a handle is not re-entrant.
 */
#ifndef GRL_H_
#define GRL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRL_OK 0
#define GRL_ERR_INVALID (-1)
#define GRL_ERR_HIP (-2)
#define GRL_ERR_STATE (-3)

#define GRL_MAX_LAYERS 4

/* feature extractor selected by sb_helper.py:85-96 */
#define GRL_EXTRACTOR_MLP 0        /* sacMlp on vector observations (auto-encoder features)      */
#define GRL_EXTRACTOR_AUGMENTED 1  /* sacCnn + custom_obs_policy.create_augmented_nature_cnn(n)  */
#define GRL_EXTRACTOR_NATURE 2     /* sacCnn with the default nature_cnn over all channels       */

#define GRL_ALGO_SAC 0   /* sb.SAC  sb_helper.py:104-128 */
#define GRL_ALGO_DQN 1   /* sb.DQN  sb_helper.py:159-165 */
#define GRL_ALGO_BDQ 2   /* sb.BDQ  sb_helper.py:210-224 */
#define GRL_ALGO_AE 3    /* depth auto-encoder training: gripperEnv/encoders.py:40-50,70-136, config/encoder.yaml */
#define GRL_ALGO_PPO 4   /* sb.PPO2 sb_helper.py:137-154; created through grl_ppo_create (grl_ppo_config below) */
#define GRL_ALGO_TRPO 5  /* sb.TRPO sb_helper.py:129-136; created through grl_trpo_create (grl_trpo_config below) */

typedef struct grl_config {
  int32_t extractor;      /* GRL_EXTRACTOR_*                                                    */
  int32_t img_hw;         /* side of the square camera image, 36 .. 128 (config/camera_info.yaml:1-2: 64).  64 runs the
                             sample-local convolution stack, every other size one implicit-GEMM launch per layer; the
                             extractor's dense kernel is [64 * o3 * o3, 512] with o1 = (hw - 8) / 4 + 1, o2 = (o1 - 4) / 2 + 1,
                             o3 = o2 - 2 (TF 'VALID', divisions floor).  grl_query_sizes / grl_create refuse a size
                             outside the range, and a size x batch whose largest buffer reaches 2^31 bytes          */
  int32_t obs_channels;   /* channels of the env observation: 2 depth, 5 RGB-D (robot.py:223-228) */
  int32_t n_direct;       /* direct features carried in the last channel (augmented only)       */
  int32_t obs_dim;        /* vector observation size (MLP extractor only).  DQN / BDQ handles: any size -- an image
                             observation is handed over flattened in C order (64 * 64 * C values, NOT divided by 255);
                             a handle whose first kernel exceeds 131 072 floats takes the wide route of plan_q.inl    */
  int32_t act_dim;        /* 5 full / 3 simplified (actuator.py:60-73)                           */
  int32_t n_layers;       /* len(config[algo]['layers'])                                        */
  int32_t layers[GRL_MAX_LAYERS];
  int32_t batch_size;     /* per-GPU minibatch                                                  */
  int32_t act_batch;      /* max observations per grl_act call (vectorised envs)                */
  int64_t replay_capacity;
  int32_t normalize;      /* config['normalize'] -> VecNormalize at sample time: 0 off, 1 observations and
                             rewards (sb_helper.py:117-119), 2 observations only (norm_reward=False),
                             3 rewards only (norm_obs=False)                                     */
  float gamma, lr, tau;
  float clip_obs, clip_reward, norm_eps;
  float target_entropy;   /* -act_dim for ent_coef='auto'                                       */
  uint64_t seed;          /* device RNG (replay indices, policy noise) when none are supplied   */
  /* ---- DQN / BDQ (algo != GRL_ALGO_SAC): vector observations, extractor must be GRL_EXTRACTOR_MLP,
     act_dim = q_branches (the replay stores one bin index per action dimension)              */
  int32_t algo;           /* GRL_ALGO_* (GRL_ALGO_PPO: see grl_ppo_config for what the fields above mean there)   */
  int32_t q_branches;     /* 1 for DQN; action dimensions for BDQ                               */
  int32_t q_bins;         /* discrete actions (DQN) / num_actions_pad per dimension (BDQ)       */
  int32_t q_n_common;  int32_t q_common[GRL_MAX_LAYERS];   /* BDQ layers[0] (shared trunk)     */
  int32_t q_n_branch;  int32_t q_branch[GRL_MAX_LAYERS];   /* hidden layers of each branch     */
  int32_t q_n_value;   int32_t q_value[GRL_MAX_LAYERS];    /* hidden layers of the value tower */
  int32_t q_huber;        /* 1: Huber loss (DQN), 0: squared TD (BDQ)                           */
  int32_t q_double;       /* double-Q action selection                                          */
  float q_grad_clip;      /* per-variable clip_by_norm (10 in stable-baselines), 0 = off        */
  float q_trunk_scale;    /* gradient scale entering the shared trunk (BDQ: 1/(D+1))            */
  /* prioritised replay on the device (`prioritized_replay: True`, gripper_grasp.yaml:102;
     stable-baselines PrioritizedReplayBuffer semantics, csrc/per_kernels.h)                       */
  int32_t q_per;          /* 1: keep priorities in the replay arena, enable grl_train_step_per  */
  float q_per_alpha;      /* prioritized_replay_alpha (0.6)                                      */
  float q_per_eps;        /* prioritized_replay_eps (1e-6)                                       */
  /* RGB-D observations (obs_channels 5 = R, G, B, depth, pad; robot.py:201-202): keep the three colour channels of
     a stored transition as bytes (the camera delivers uint8, sensor.py:126-145) -- one packed dword + one float32
     depth per pixel, 32 KB per observation instead of 64 KB, so that the reference's 1 M-transition buffer
     (full_depth_obs.yaml / SAC_full_rgbd) is 65.5 GB of HBM.  Lossless iff the colour values are integers in
     [0, 255]; the caller vouches for that.  Requires 4 image channels (augmented extractor on 5-channel obs). */
  int32_t replay_rgb_u8;
  /* prioritised replay, continued.  q_per_stratified: 0 = stable-baselines 2.10.x `_sample_proportional`
     (mass = np.random.random(size=batch) * total; the version setup.py:7-12 pins), 1 = the stratified form of
     OpenAI baselines / stable-baselines < 2.10 (mass_k = random() * L + k * L, L = total / batch).
     q_per_alpha64: prioritized_replay_alpha as the Python float the reference passes (the exponent of
     `max_priority ** alpha` at add time; q_per_alpha is its float32 rounding, the exponent NumPy uses for the
     float32 priorities of an update); 0 = use q_per_alpha. */
  int32_t q_per_stratified;
  double q_per_alpha64;
  /* BDQ: the `bdq_sb` fork's source is not available (.gitmodules:1-3, no pinned commit), so two aggregation choices of
     its update are switches rather than citations (oracle/dqn.py): q_loss_sum_branches = 1 sums the squared TD errors
     over the action branches instead of averaging them (default 0: mean, Tavakoli et al. 2018 eq. 6);
     q_trunk_scale above = 1 disables the 1/(D+1) rescaling of the gradient entering the shared trunk. */
  int32_t q_loss_sum_branches;
  /* DQN / BDQ: 1 = layer normalisation in front of the ReLU of every HIDDEN layer of the Q-network (stable-baselines
     `LnMlpPolicy` / policy_kwargs layer_norm=True: tf.contrib.layers.layer_norm, epsilon 1e-12, csrc/ln_kernels.h); the
     parameter table then holds `LayerNorm[_k]/beta:0` and `LayerNorm[_k]/gamma:0` behind the layer's weights and biases.
     Appended last: it occupies what used to be the struct's tail padding, so every earlier field and sizeof(grl_config)
     stay where they were -- a caller that does not zero the struct now has to set it.  Must be 0 on SAC handles. */
  int32_t q_layer_norm;
  /* Auto-encoder handles (algo 3): the network of encoders.py:85-124 as config/encoder.yaml describes it -- three encoder
     layers of stride 2 on a 64x64x1 image with `ae_kernel[l]` (1..9, TensorFlow 'SAME' borders) and `ae_filters[l]` (a multiple
     of 4 in 4..64), a bottleneck of `ae_encoding_dim` (1..1024) and LeakyReLU slope `ae_alpha` (0 <= alpha < 1); the decoder
     mirrors it.  ALL of them zero: the shipped network (7/5/3, 32/32/32, 100, 0.1), which runs the tuned launch plan; any
     other supported network runs the general one.  Otherwise every field is taken as written.  Appended
     last: earlier fields keep their offsets, sizeof(grl_config) grows by 32 bytes (a caller built against the earlier header has
     to be rebuilt; grl_state_import still takes blobs that hold the shorter struct).  Must all be 0 on handles of another algo. */
  int32_t ae_kernel[3];
  int32_t ae_filters[3];
  int32_t ae_encoding_dim;
  float ae_alpha;
} grl_config;

/* byte sizes of the four caller-provided device arenas */
typedef struct grl_sizes {
  size_t state_bytes;   /* parameters (incl. target net), Adam moments, scalars                 */
  size_t grads_bytes;   /* flat fp32 gradient bucket (the data-parallel all-reduce payload)     */
  size_t work_bytes;    /* activations, gradient workspaces, descriptor tables                  */
  size_t replay_bytes;  /* replay ring: obs, next_obs, action, reward, done                     */
  int64_t n_params;     /* floats in the parameter block (trainable + target, incl. padding)    */
  int64_t n_trainable;  /* floats covered by the gradient bucket                                */
} grl_sizes;

typedef struct grl_buffers {
  void* state;
  void* grads;
  void* work;
  void* replay;
} grl_buffers;

/* losses / diagnostics of one update, as logged by SB (logs.csv columns) */
typedef struct grl_metrics {
  float policy_loss, qf1_loss, qf2_loss, value_loss, ent_coef_loss, ent_coef, entropy;
  float mean_qf1, mean_v;
} grl_metrics;

typedef struct grl_ctx* grl_handle;

const char* grl_last_error(void);
int grl_version(void);

int grl_query_sizes(const grl_config* cfg, grl_sizes* out);
int grl_create(const grl_config* cfg, const grl_buffers* bufs, grl_handle* out);
int grl_destroy(grl_handle h);
int grl_set_stream(grl_handle h, void* hip_stream);

/* parameter layout: TF variable names (with ":0") in TF creation order, as in the SB zips */
int grl_param_count(grl_handle h);
int grl_param_info(grl_handle h, int index, char* name, int name_cap, int64_t* offset_floats,
                   int64_t* numel, int32_t* ndim, int64_t shape[4], int32_t* trainable);
/* re-initialise Adam moments / beta powers (after load_parameters) */
int grl_reset_optimizer(grl_handle h);

/* learning rate of the following updates (stable-baselines evaluates `learning_rate(progress)` before every
   update when a schedule is given; a constant needs no call: updates start with cfg.lr).  Takes effect in
   stream order; captured graphs stay valid (the value lives in device memory). */
int grl_set_learning_rate(grl_handle h, float lr);

/* VecNormalize statistics (host float64, HWC layout of the observation space or [obs_dim]);
   obs_var/ret_var are variances, epsilon is added inside.  Copied before returning. */
int grl_set_obs_stats(grl_handle h, const double* obs_mean, const double* obs_var, double ret_var);
/* The same statistics maintained ON THE DEVICE (SAC, DQN and BDQ handles; PPO / TRPO handles created with normalize = 2 keep the
   OBSERVATION statistics the same way, see grl_observe and the PPO2 block: grl_set_running_stats and grl_get_obs_stats work on
   them as described here, grl_set_obs_stats loads mean / var and ignores ret_var, grl_norm_update is GRL_ERR_STATE; on a
   normalize = 0 PPO / TRPO handle all of them are GRL_ERR_STATE).  VecNormalize.step_wait -> obs_rms.update(obs)
   (stable-baselines RunningMeanStd.update / update_from_moments, wrapper created at sb_helper.py:117-119): merges the
   batch moments of the n raw observations of one env step (HOST pointer, env layout [n, 64, 64, C+1] or [n, obs_dim],
   n <= max(act_batch, 64)) into the running mean / variance / count in device memory -- float32 batch moments like
   NumPy forms them from the float32 observations, float64 Chan merge -- and refreshes the sample-time statistics;
   stream-ordered, no synchronisation.  grl_set_running_stats loads a starting point for them (the mean / var / count of a
   vecnormalize.pkl; RunningMeanStd starts at 0 / 1 / 1e-4) -- grl_set_obs_stats only loads what sampling reads --
   grl_set_ret_var pushes the host-side return variance alone, and grl_get_obs_stats (host, synchronises) copies
   mean / var [env layout] and count out for pickling.
   On a handle connected for data parallelism (grl_allreduce_connect) grl_norm_update merges the batch moments of ALL
   ranks, in rank order, into every replica (csrc/dp_kernels.h) -- the arithmetic of
   grasp_rl.parallel.share_running_stats on the host; all ranks must call it the same number of times.  That merge is the
   SAC handles': on a connected DQN / BDQ handle grl_norm_update and grl_observe(GRL_OBSERVE_UPDATE_STATS) are GRL_ERR_STATE
   before anything moves (keep the statistics on the host there). */
int grl_norm_update(grl_handle h, const float* obs, int n);
int grl_set_running_stats(grl_handle h, const double* obs_mean, const double* obs_var, double count);
int grl_set_ret_var(grl_handle h, double ret_var);
int grl_get_obs_stats(grl_handle h, double* obs_mean, double* obs_var, double* count);

/* append n raw (un-normalised) transitions; host pointers, obs in env layout [n,H,W,C] or [n,D] */
int grl_replay_add(grl_handle h, const float* obs, const float* act, const float* rew,
                   const float* next_obs, const float* done, int n);
/* same, device pointers already on the stream */
int grl_replay_add_device(grl_handle h, const float* obs, const float* act, const float* rew,
                          const float* next_obs, const float* done, int n);
int64_t grl_replay_size(grl_handle h);

/* n_steps updates.  idx [n_steps*batch] int64 replay indices and eps [n_steps*batch*act_dim]
   standard-normal noise are DEVICE pointers; pass NULL to draw them on the device (Philox).
   DQN / BDQ handles: `eps` carries the prioritised-replay importance weights [n_steps*batch]
   (NULL with idx == NULL: uniform sampling on the device, weights 1). */
int grl_train_step(grl_handle h, int n_steps, const int64_t* idx, const float* eps);
/* DQN / BDQ with q_per (stable-baselines DQN.learn with prioritized_replay=True: replay_buffer.sample(batch_size,
   beta=...) -> _train_step(importance weights) -> update_priorities(|td| + eps)): n_steps updates on minibatches drawn
   proportionally to the float64 leaves priority**alpha (csrc/per_kernels.h restates the segment-tree arithmetic),
   importance weights (N p)^-beta / max, then leaves <- float32(|td| + eps) ** float32(alpha).  beta > 0, at least two
   stored transitions.  u_or_null: DEVICE pointer to [n_steps*batch] float64 uniforms in [0,1) (what np.random.random
   delivers; parity tests); NULL = device Philox, 53 bits per draw. */
int grl_train_step_per(grl_handle h, int n_steps, double beta, const double* u_or_null);
/* DQN / BDQ: hard copy of the online network into the target network (target_network_update_freq) */
int grl_q_update_target(grl_handle h);
/* split form for data parallelism: grads -> (caller all-reduces the grads arena) -> apply */
int grl_compute_grads(grl_handle h, const int64_t* idx, const float* eps);
int grl_apply_grads(grl_handle h, float grad_scale);
/* The same gradient computation in two stages, for overlapping the exchange with compute: after
   stage 0 the ranges of bucket 0 (fully-connected + head layers: ~90 % of the bytes) are final in the grads arena,
   after stage 1 those of bucket 1 (convolutions, entropy coefficient).  Typical use: stage 0 -> start all-reduce of
   bucket 0 on a second stream -> stage 1 -> all-reduce bucket 1 -> grl_apply_grads.  idx / eps as for
   grl_compute_grads (stage 0 only).  Handles without a staged plan (vector observations, DQN / BDQ) do everything
   in stage 0 and report one range covering the whole bucket. */
int grl_compute_grads_staged(grl_handle h, int stage, const int64_t* idx, const float* eps);
/* The exchange step inside the library (csrc/dp_kernels.h): all-reduces written for this path over exchange
   buffers that every rank exports with hipIpcGetMemHandle and maps from its peers (xGMI between the GPUs of a node).
   The gradient computation's last launch publishes the sums it forms; then either TWO-SHOT -- reduce-scatter by the owner
   of each 1/world chunk in rank order, all-gather by pull inside the Adam kernel -- or ONE-SHOT (small worlds) -- every
   rank adds all contributions in rank order inside the Adam kernel.
     grl_allreduce_init     allocates this rank's exchange memory -- a few hundred bytes of flags and a
                            buffer of three bucket-sized arrays + two moment blocks, both fine-grained (the only device
                            memory the library allocates itself: IPC export needs allocations of its own) -- and writes
                            their two IPC handles, GRL_ALLREDUCE_HANDLE_BYTES = 128 bytes, to handle_out; the host
                            exchanges the handles of all ranks out of band (any transport: files, MPI,
                            torch.distributed.all_gather_object);
     grl_allreduce_connect  handles = world x GRL_ALLREDUCE_HANDLE_BYTES in rank order; maps the peers' memory;
     grl_allreduce_disconnect   host (synchronises this handle's stream): unmaps the peers, frees the exchange memory, and
                            the handle is a single-process handle again (grl_norm_update / grl_observe no longer merge over
                            ranks; grl_allreduce_init may be called anew).  For a set-up that failed on SOME rank -- every
                            rank then releases what it had and the job falls back together -- and for an orderly end of
                            training.  The caller guarantees that no exchange is in flight on any rank (drain, barrier).
                            No-op on a handle that was never initialised;
     grl_train_step_allreduce   n_steps data-parallel updates, each ONE graph: minibatch from this rank's replay shard,
                            gradients, exchange, Adam + Polyak with the mean gradient -- what grl_compute_grads ->
                            all-reduce -> grl_apply_grads(1 / world) does with a collective library in between.  Every
                            replica receives bit-identical sums.  All ranks must call it the same number of times.  A rank
                            WAITS for a peer that is late (GRL_TUNE dp_timeout_ms, default 120 s); when a wait runs out the
                            rank poisons the channel on every rank: this and every later call fail with GRL_ERR_STATE on
                            all of them (no replica keeps training on a partial exchange);
     grl_allreduce_status   host (synchronises): exchanges begun; error != 0 (and a negative return) after a time-out;
     grl_allreduce_set_mode 0 (default): one-shot for world <= 2, else two-shot; 1: two-shot; 2: one-shot.  All ranks must
                            choose alike, while no exchange is in flight on any rank;
     grl_allreduce_set_timeout   host, any time: bound of every wait for a peer in milliseconds from now on (0 = back to the
                            default, GRL_TUNE dp_timeout_ms or 120 s) -- short while a freshly set-up exchange is being
                            verified (a channel that cannot work should cost seconds, not minutes: bench.py's
                            make_data_parallel), long while training (a peer running an evaluation callback is merely late).
                            Takes effect for waits already in progress; values below 200 ms act as 200 ms;
     grl_allreduce_set_overlap   on = 1: grl_train_step_allreduce runs the staged plan (grl_compute_grads_staged) with BOTH
                            exchanges in its graph -- bucket 0 (dense layers, ~90 % of the bytes) is reduced and exchanged on
                            a side lane of the graph while the backward through the convolutions runs, bucket 1 follows,
                            Adam waits for both (SURVEY.md 8e "overlapped with the backward"; two-shot).  Same sums,
                            bit-identical parameters.  All ranks must choose alike.  GRL_ERR_STATE when the handle has no
                            staged plan (vector observations); off by default.
   DQN / BDQ handles (uniform replay) take part the same way: tf.clip_by_norm per variable sits between the all-reduce and
   Adam there, so their exchange is two-shot + a pull of every sum into the gradient bucket, followed by the plan's own clip +
   Adam with grad_scale 1 / world -- the SUM is clipped at world x clip, i.e. the MEAN of the replicas is clipped as one
   gradient (the same holds for grl_compute_grads -> all-reduce -> grl_apply_grads(1 / world)).  Mode 2 and the overlapped
   form are GRL_ERR_STATE on them.  Prioritised handles keep per-rank priority trees: on a connected handle
   grl_train_step_per draws from this rank's tree (importance weights against its own total and minimum), exchanges the
   gradient sums the same way and writes the priorities of its own rows back; grl_train_step_allreduce (uniform draws) is
   GRL_ERR_STATE on them.  All ranks call alike. */
#define GRL_ALLREDUCE_HANDLE_BYTES 128
int grl_allreduce_init(grl_handle h, int rank, int world, void* handle_out);
int grl_allreduce_connect(grl_handle h, const void* handles);
int grl_allreduce_disconnect(grl_handle h);
int grl_allreduce_set_overlap(grl_handle h, int on);
int grl_allreduce_set_mode(grl_handle h, int mode);
int grl_allreduce_set_timeout(grl_handle h, int ms);
int grl_train_step_allreduce(grl_handle h, int n_steps, const int64_t* idx, const float* eps);
int grl_allreduce_status(grl_handle h, int64_t* exchanges, int* error);
/* contiguous ranges (float offsets into the grads arena) of bucket 0 / 1; returns their number (<= cap) or < 0 */
int grl_grad_ranges(grl_handle h, int bucket, int cap, int64_t* offsets, int64_t* numels);
/* host: metrics of the most recent update (synchronises the stream) */
int grl_get_metrics(grl_handle h, grl_metrics* out);

/* host: actor forward for n <= act_batch observations (env layout, host ptr); `flags` is a mask of the bits below
   (any other bit: GRL_ERR_INVALID).
     GRL_ACT_DETERMINISTIC  tanh(mu) instead of a sample;
     GRL_ACT_RAW_OBS        (SAC handles; DQN / BDQ handles with GRL_ACT_GREEDY) the observations are RAW and VecNormalize.normalize_obs is applied on the device
                            with the statistics grl_norm_update / grl_observe maintain (otherwise they are already
                            normalised, as VecNormalize hands them out).  On a DQN / BDQ handle a NaN observation stays a
                            NaN, as np.clip leaves it;
     GRL_ACT_OBSERVED       (SAC handles; DQN / BDQ handles with GRL_ACT_GREEDY) act on the n observations the last grl_observe uploaded; `obs` is ignored
                            (may be NULL) and nothing but eps and the actions crosses the bus; GRL_ERR_STATE when n differs
                            from the rows held.
   eps_or_null: [n,act_dim] noise for stochastic actions (host).  Synchronises the stream.
   DQN / BDQ handles: out receives the dueling Q-values [n, q_branches*q_bins] (normalised observations only:
   GRL_ACT_RAW_OBS / GRL_ACT_OBSERVED are GRL_ERR_STATE in this form), or with
     GRL_ACT_GREEDY         (DQN / BDQ handles; GRL_ERR_STATE on the others) the epsilon-greedy ACTION of every row: out
                            receives the bins [n, q_branches] as float32 -- the arg-max of the Q-values over the bins of each
                            branch (lowest index among equal values, as np.argmax), formed on the device -- and eps_or_null
                            is the exploration table explore[n, q_branches] (host) or NULL (all greedy): an entry >= 0
                            replaces the greedy bin of that (row, branch) and comes back verbatim, a negative entry keeps
                            it.  The caller draws the randomness.  Combines with GRL_ACT_RAW_OBS and GRL_ACT_OBSERVED, each
                            with the meaning above (the one-launch kernel then normalises the rows while it stages them).
                            One launch for networks whose widths and bins fit 64,
                            observations up to 128 values and up to 7 branches (csrc/q_act.h); other shapes run the launches
                            of the Q-value path plus a select launch.  Stands behind stable-baselines DQN.learn's
                            `self.act(...)` as entered from sb_helper.py:159-177 and `model.predict` in utils.py:71. */
#define GRL_ACT_DETERMINISTIC 1
#define GRL_ACT_RAW_OBS 2
#define GRL_ACT_OBSERVED 4
#define GRL_ACT_GREEDY 8
int grl_act(grl_handle h, const float* obs, int n, int flags, const float* eps_or_null,
            float* out_actions);

/* One env step's observations uploaded ONCE (SAC, DQN and BDQ handles; on the latter two `act` holds the chosen bins
   [n, q_branches] as float32).  In SAC.learn the observations an env step returns are used
   three times -- RunningMeanStd.update (VecNormalize.step_wait), the next model.predict-style action, and two
   replay_buffer.add rows (new_obs of this step, obs of the next; stable-baselines' learn loop entered at
   sb_helper.py:175-177).  grl_observe copies obs [n, env layout] (host ptr, n <= max(act_batch, 64); copied before the
   call returns) to the device, keeps the previous call's observations beside them and, with GRL_OBSERVE_UPDATE_STATS,
   folds them into the running statistics exactly as grl_norm_update does.  grl_act(GRL_ACT_OBSERVED) then acts on them;
   grl_replay_add_observed appends the n transitions (previous observations, act, rew, newest observations, done) --
   GRL_ERR_STATE unless the last two grl_observe calls both held n observations.  Rows whose episode ended store the
   terminal observation instead: term_rows [n_term] names them, term_obs [n_term, env layout] holds their observations
   (the auto-resetting VecEnv has already put the next episode's first observation in the observed row).
   All stream-ordered; nothing synchronises.
   PPO / TRPO handles created with normalize = 2: n must equal n_envs (GRL_ERR_INVALID otherwise).  The raw rows are uploaded once
   and ONE launch (ppo_observe_kernel) folds them into the running statistics (with GRL_OBSERVE_UPDATE_STATS; without it the
   statistics stay) and writes VecNormalize.normalize_obs of every row, float32, with the statistics as they stand after that
   update -- what stable-baselines stores in a PPO rollout -- into the rows grl_ppo_step / grl_ppo_finish read when their obs is
   NULL.  A NaN observation stays a NaN.  grl_replay_add_observed is GRL_ERR_STATE on these handles. */
#define GRL_OBSERVE_UPDATE_STATS 1
int grl_observe(grl_handle h, const float* obs, int n, int flags);
int grl_replay_add_observed(grl_handle h, const float* act, const float* rew, const float* done, int n,
                            const int32_t* term_rows, const float* term_obs, int n_term);

/* GRL_ALGO_AE handles: n_steps minibatch updates of the depth auto-encoder (forward, mean-squared
   reconstruction error, backward, Keras-Adam; encoders.py:40-50,127-136).  imgs: DEVICE pointer to
   [n_steps*batch_size, 64, 64, 1] float32 depth images (train_encoder.py:19-27 preprocessing is the
   caller's).  Parameters are the 16 Keras tensors of model.h5 (grl_param_info); grl_get_metrics reports
   the reconstruction loss of the last minibatch in policy_loss; grl_encode works on the handle. */
int grl_ae_train_step(grl_handle h, const float* imgs, int n_steps);

/* GRL_ALGO_AE handles: forward pass only (Keras Model.predict, encoders.py:52-57 `test` / `predict`): the
   reconstruction of one minibatch.  imgs, out: DEVICE pointers to [batch_size, 64, 64, 1] float32.
   Parameters and optimiser state are untouched. */
int grl_ae_reconstruct(grl_handle h, const float* imgs, float* out);

/* Keras depth auto-encoder (encoder half).  weights: 8 host arrays in Keras order
   conv2d_1..3 kernel(HWIO)/bias, dense_1 kernel [2048,100]/bias; copied into the work arena. */
int grl_encoder_load(grl_handle h, const float* const* weights, const int64_t* numels, int n_arrays);
/* host: depth [n,64,64,1] float32 -> out [n,100]; n <= act_batch.  Synchronises the stream. */
int grl_encode(grl_handle h, const float* depth, int n, float* out_feat);

/* ---------------------------------------------------------------------------------------------------------------------
   PPO2 (GRL_ALGO_PPO): stable-baselines 2.10.1 PPO2 with the actor-critic MlpPolicy on a Box action space, as
   sb_helper.py:137-154 builds it.  The handle is described by a grl_config AND a grl_ppo_config and is created through the two
   calls below (grl_query_sizes / grl_create return GRL_ERR_INVALID for algo 4 and name them).  In the grl_config of such a handle
   extractor is GRL_EXTRACTOR_MLP; obs_dim (observations of any rank flattened in C order, not divided by 255), act_dim and seed
   mean what they say; n_layers / layers[] describe the pi tower (tanh, widths 1..1024); batch_size is the minibatch row count;
   act_batch equals n_envs; replay_capacity is R = n_envs * n_steps; gamma and lr mean what they say; every q_*,
   ae_* and replay_rgb_u8 field is 0.  normalize is 0 (the handle is handed normalised observations) or 2: the handle also
   keeps VecNormalize's observation statistics in float64 -- running mean / var [obs_dim] and count, starting at 0 / 1 / 1e-4,
   and sqrt(var + eps) -- the raw rows of one env step and their normalised form [n_envs, rup(obs_dim, 4)] (grl_observe;
   clip_obs and norm_eps are read, the epsilon as grl_ppo_config.norm_eps64 when that is set).  1 and 3 are GRL_ERR_INVALID:
   they normalise rewards at sample time, and a rollout stores the reward VecNormalize normalised at step time, on the host.
   A normalize = 0 handle is what it was before the value 2 existed: arena sizes, plan and launches.  The four arenas keep their roles; the rollout lives in the replay arena.
   Parameters (grl_param_info), TF creation order: model/pi_fc<l>/{w,b}:0 and model/vf_fc<l>/{w,b}:0 with the layer index
   outermost, model/vf/{w,b}:0, model/pi/{w,b}:0, model/pi/logstd:0 [1, A], model/q/{w,b}:0 (initialised, never read, not trainable). */
typedef struct grl_ppo_config {
  int32_t n_envs, n_steps;                 /* R = n_envs * n_steps rollout rows; grl_config.batch_size must divide R */
  int32_t n_vf_layers; int32_t vf_layers[GRL_MAX_LAYERS];
  float lam, clip_range, clip_range_vf;    /* clip_range_vf < 0: no value clipping */
  float ent_coef, vf_coef, max_grad_norm;  /* max_grad_norm <= 0: no clipping */
  float adam_eps;                          /* 1e-5 */
  double norm_eps64;                       /* normalize = 2: VecNormalize's epsilon as the Python float it is (1e-8 is no float32);
                                              0: grl_config.norm_eps widened */
} grl_ppo_config;
int grl_ppo_query_sizes(const grl_config* cfg, const grl_ppo_config* ppo, grl_sizes* out);
int grl_ppo_create(const grl_config* cfg, const grl_ppo_config* ppo, const grl_buffers* bufs, grl_handle* out);

/* model.step: n == n_envs rows. obs [n, obs_dim], done [n] (flags from before the step), eps_or_null [n, A] are host pointers
   (NULL: device Philox from cfg.seed). Writes obs / action / value / neglogp / done into slot t of the rollout on the device
   and copies action (unclipped), value, neglogp to the host outputs; synchronises. GRL_ERR_STATE when the rollout is full or the
   previous slot has not been closed by grl_ppo_rewards.  obs == NULL (grl_ppo_finish: last_obs == NULL) means "the rows the last
   grl_observe normalised": GRL_ERR_STATE when there are none or the handle has normalize = 0; a non-NULL obs is taken as
   already normalised. */
int grl_ppo_step(grl_handle h, const float* obs, const float* done, const float* eps_or_null,
                 float* out_act, float* out_val, float* out_nlp);
int grl_ppo_rewards(grl_handle h, const float* rew, int n);                     /* closes slot t; stream-ordered */
/* model.value(last obs) + GAE over the full rollout -> adv, ret on the device; GRL_ERR_STATE unless n_steps slots are closed */
int grl_ppo_finish(grl_handle h, const float* last_obs, const float* last_done);
/* noptepochs * (R / batch_size) updates. perm: host int32 [noptepochs, R], each row a permutation of 0..R-1 (checked:
   GRL_ERR_INVALID names the first row that is none); 1 <= noptepochs <= GRL_PPO_MAX_EPOCHS. Needs a finished rollout
   (GRL_ERR_STATE otherwise) and empties it. Stream-ordered, no synchronisation. */
#define GRL_PPO_MAX_EPOCHS 64
int grl_ppo_train(grl_handle h, const int32_t* perm, int noptepochs);
/* host, synchronises: the five diagnostics (policy loss, value loss, entropy, approxkl, clipfrac) of every update of the last
   grl_ppo_train call, [n_updates, 5]; returns n_updates, GRL_ERR_INVALID when cap (in floats) is too small */
int grl_ppo_get_metrics(grl_handle h, float* out, int cap);
/* On a PPO handle grl_act (n <= act_batch rows; GRL_ACT_DETERMINISTIC: the mean, else a sample -- eps_or_null NULL draws on the
   device; unclipped; records nothing; the other flags are GRL_ERR_STATE), grl_param_count / _info, grl_reset_optimizer,
   grl_set_learning_rate, grl_set_stream, grl_profile_*, grl_ppo_state_size / _export / _import (checkpoints, below) and
   grl_debug_fetch / _store work; the debug names are "ppo_obs" [R, ld],
   "ppo_act", "ppo_old_v", "ppo_old_nlp", "ppo_rew", "ppo_done", "ppo_adv", "ppo_ret" (rollout, row = env * n_steps + t),
   "ppo_last_v", "ppo_last_done", "ppo_mean", "ppo_v" (the last minibatch), "ppo_slots" (grl_debug_store only, three values: slots written,
   slots closed, finished -- says how far a rollout placed through the other names has got), "grads", "adam_m", "adam_v", and with
   normalize = 2 "ppo_obs_n" [n_envs, ld] (the rows the last grl_observe normalised).  Every other entry point returns
   GRL_ERR_STATE on a PPO handle before anything moves (normalize = 2: but for grl_observe and the three statistics calls).
   grl_act is the same on both kinds of handle: the observations handed to it are taken as normalised. */

/* ---------------------------------------------------------------------------------------------------------------------
   TRPO (GRL_ALGO_TRPO): stable-baselines 2.10.1 TRPO with the actor-critic MlpPolicy on a Box action space, as
   sb_helper.py:129-136 builds it: ONE environment, a rollout of n_steps = timesteps_per_batch rows, one natural-gradient policy
   step (conjugate gradient on the Fisher-vector product over every fvp_stride-th row, backtracking line search) and the Adam fit
   of the value tower per rollout.  The handle is described by a grl_config AND a grl_trpo_config.  The grl_config is read as on
   a PPO handle with lr = vf_stepsize, act_batch = 1, batch_size = vf_batch and replay_capacity = n_steps; parameters and their
   order are those of a PPO handle.  The policy variables are those whose name contains "/pi"; every other trainable variable
   belongs to the value fit.
   Rollout: grl_ppo_step / grl_ppo_rewards / grl_ppo_finish work on a TRPO handle with n_envs = 1 (done = episode_start of the
   step; grl_ppo_finish forms V(last obs), GAE and tdlamret).  normalize = 2, grl_observe, the statistics calls and obs == NULL
   work as on a PPO handle (one row).  grl_ppo_train / grl_ppo_get_metrics are GRL_ERR_STATE. */
typedef struct grl_trpo_config {
  int32_t n_steps;                         /* T = timesteps_per_batch, 1 .. 65536 */
  int32_t n_vf_layers; int32_t vf_layers[GRL_MAX_LAYERS];
  int32_t cg_iters;                        /* 1 .. 64 */
  int32_t ls_steps;                        /* line-search trials 2^-0 .. 2^-(ls_steps - 1): 1 .. 16 (stable-baselines: 10) */
  int32_t fvp_stride;                      /* the Fisher rows are 0, fvp_stride, 2 fvp_stride, ... (stable-baselines: 5) */
  int32_t vf_batch;                        /* rows of a value minibatch (stable-baselines: 128); must equal grl_config.batch_size */
  float lam, max_kl, cg_damping, ent_coef;
  float adam_eps;                          /* 1e-8 */
  double norm_eps64;                       /* as grl_ppo_config.norm_eps64 */
} grl_trpo_config;
int grl_trpo_query_sizes(const grl_config* cfg, const grl_trpo_config* trpo, grl_sizes* out);
int grl_trpo_create(const grl_config* cfg, const grl_trpo_config* trpo, const grl_buffers* bufs, grl_handle* out);
/* One learn iteration behind a finished rollout (GRL_ERR_STATE otherwise; empties it): advantage standardisation, losses and
   gradient at the old parameters, cg_iters Fisher products, the closing product for shs, ls_steps trials, restore, then
   vf_iters * floor(T / vf_batch) Adam minibatches of the value tower.  vf_perm: host int32 [vf_iters, T], each row a permutation
   of 0..T-1 (checked as grl_ppo_train checks; row e's minibatch k takes its entries [k vf_batch, (k + 1) vf_batch), the tail is
   dropped); 0 <= vf_iters <= GRL_PPO_MAX_EPOCHS (0: vf_perm may be NULL).  The launch list has a fixed shape -- a launch whose
   device flag says "CG finished" / "trial accepted" returns at once.  Stream-ordered, no synchronisation. */
int grl_trpo_update(grl_handle h, const int32_t* vf_perm, int vf_iters);
/* host, synchronises: GRL_TRPO_METRICS floats of the last grl_trpo_update: [0..4] optimgain, meankl, entbonus, surrgain, meanent
   before the step; [5] accepted line-search index (-1: parameters restored, -2: zero gradient, no step); [6], [7] optimgain and
   meankl of the accepted trial (0 without one); [8] conjugate-gradient iterations run; [9] the final r.r; [10] shs. */
#define GRL_TRPO_METRICS 11
int grl_trpo_get_metrics(grl_handle h, float* out, int cap);
/* parity: F(v) of the vector stored under "trpo_fvp_in" at the current parameters over the Fisher rows of the rollout on the
   device, left under "trpo_fvp_out"; needs a full rollout (slots closed).  The entries of the value variables in the stored
   vector must be zero (they are in every vector an update forms).  Stream-ordered. */
int grl_trpo_debug_fvp(grl_handle h);
/* grl_act, grl_param_*, grl_reset_optimizer, grl_set_learning_rate, grl_set_stream, grl_profile_*, grl_ppo_state_size /
   _export / _import and grl_debug_fetch / _store work as on a PPO handle.  Debug names: those of the PPO rollout, and -- laid out like the gradient bucket ([n_trainable], the
   entries of the value variables 0) -- "trpo_g", "trpo_stepdir", "trpo_fullstep", "trpo_fvp_in", "trpo_fvp_out",
   "trpo_theta_old" (every trainable variable as it was when the update began); "trpo_atarg" [T]; "trpo_mean_old" [T, A] (the
   old policy's means).  The grl_gail_* calls (below) open a GAIL session on a TRPO handle.  Every other entry point returns
   GRL_ERR_STATE on a TRPO handle before anything moves. */

/* ---------------------------------------------------------------------------------------------------------------------
   TD3 (GRL_ALGO_TD3): stable-baselines 2.10.1 TD3 (td3/td3.py, td3/policies.py) with MlpPolicy on a Box action space: a
   deterministic policy pi = tanh(dense(relu-MLP(obs))), twin critics on [obs, action], target copies of all three.  The handle
   is described by a grl_config AND a grl_td3_config.  The grl_config is read as on a SAC handle with GRL_EXTRACTOR_MLP: obs_dim,
   act_dim, layers, batch_size, act_batch, replay_capacity, normalize, gamma, lr, tau, clip_obs / clip_reward / norm_eps and seed
   (target_entropy is ignored; every q_* field and replay_rgb_u8 must be 0).  Parameters, in TF creation order:
   model/pi/fc{l}, model/pi/dense, model/values_fn/qf1/fc{l}, model/values_fn/qf1/qf1, the same for qf2 (all trainable), then the
   same tree under target/.
   One update on minibatch rows s, a, r, s', d (gathered and normalised as on a SAC handle):
     a' = clip(pi_target(s') + clip(sigma eps, -c, c), -1, 1);   y = r + (1 - d) gamma min(q1_target(s', a'), q2_target(s', a'))
     qf1_loss = mean((y - q1(s, a))^2), qf2_loss likewise; the critics step on their sum with an Adam of their own (epsilon 1e-8)
   and, on a policy update only: policy_loss = -mean(q1(s, pi(s))) steps model/pi with a second Adam whose step count advances
   on policy updates only, then target <- (1 - tau) target + tau online over every model/ variable.  Every gradient and metric is
   formed at the parameters the update began with; both Adam steps follow; the Polyak average reads the stepped parameters. */
#define GRL_ALGO_TD3 6   /* created through grl_td3_create (grl_td3_config) */
typedef struct grl_td3_config {
  int32_t policy_delay;                    /* >= 1: update u of a call is a policy update iff (first_step + u) % policy_delay == 0 */
  float target_policy_noise;               /* sigma >= 0 */
  float target_noise_clip;                 /* c >= 0 */
} grl_td3_config;
int grl_td3_query_sizes(const grl_config* cfg, const grl_td3_config* td3, grl_sizes* out);
int grl_td3_create(const grl_config* cfg, const grl_td3_config* td3, const grl_buffers* bufs, grl_handle* out);
/* n_updates (1 .. GRL_TD3_MAX_UPDATES) updates, stream-ordered.  idx: DEVICE int64 [n_updates, batch_size] replay rows, or NULL:
   drawn on the device (Philox: cfg.seed, one counter per update); eps: DEVICE float32 [n_updates, batch_size, act_dim] standard
   normals of the target smoothing, or NULL: drawn on the device with the same counter.  Either may be NULL.  With both NULL the
   updates go out in hipGraphs of up to `graph_updates` updates (GRL_TUNE); one call of n updates equals n calls of one update,
   bit for bit.  first_step >= 0: the learner's step count at update 0 (TD3._train_step's `step + grad_step`). */
#define GRL_TD3_MAX_UPDATES 1024
int grl_td3_train(grl_handle h, int n_updates, const int64_t* idx_or_null, const float* eps_or_null, int64_t first_step);
/* host, synchronises: [n, 6] floats of the last grl_td3_train call, one row per update: qf1_loss, qf2_loss, policy_loss (the last
   policy update's value on a critic-only update -- of this call or of any call before it, fetched or not: the value is kept on
   the device; 0 before the handle's first policy update), mean q1(s, a), mean q2(s, a), 1 if the update was a policy update else 0.
   Returns n. */
#define GRL_TD3_METRICS 6
int grl_td3_get_metrics(grl_handle h, float* out, int cap);
/* On a TD3 handle grl_replay_add / _add_device / _size, grl_set_obs_stats, grl_set_running_stats, grl_set_ret_var,
   grl_norm_update, grl_get_obs_stats, grl_param_count / _info, grl_reset_optimizer (both Adams), grl_set_learning_rate (one value
   for both), grl_set_stream, grl_profile_* and grl_debug_fetch / _store work as on a SAC handle; grl_act returns pi(obs) for
   n <= act_batch rows (GRL_ACT_DETERMINISTIC changes nothing, eps is not read: exploration noise is the host's).  Debug names:
   "td3_a_next" [B, A], "td3_noise" [B, A] (the standard normals as drawn or handed over), "td3_backup" [B], "td3_q" [5, B]
   (q1, q2, q1_target, q2_target, q1(s, pi(s))), "td3_pi" [B, A], "td3_da" [B, A], "td3_xs" / "td3_xn" [B, ld] (the critics'
   input rows [obs | action | padding] of s and s'), "rew", "done", "td3_beta_c" / "td3_beta_pi" (the beta powers of the two
   Adams), "grads", "adam_m", "adam_v".  Every other entry point returns GRL_ERR_STATE on a TD3 handle before anything moves. */

/* ---- Behaviour-cloning pretraining of a SAC handle's policy from recorded (observation, action) pairs: stable-baselines
   2.10.1 BaseRLModel.pretrain with SAC._get_pretrain_placeholders.  One update on a minibatch of n present rows:
     det = tanh(mu(obs));  a_env = low + 0.5 (det + 1)(high - low);  loss = mean over the n * act_dim elements of (a_exp - a_env)^2
   Trained: model/pi without its log-std head (model/pi/dense_1); with a CNN policy pi's own extractor too.  Everything else --
   the log-std head, the critics, the value and target networks, log_ent_coef, the SAC optimiser's moments and beta powers,
   the Philox counters, the replay ring, the running statistics -- stays bit-unchanged.  Observations are used as the table
   holds them (images divided by 255 as in the SAC update; VecNormalize statistics are never applied).  The optimiser is
   TF-1 Adam with the session's own zero moments and fresh beta powers.  A session is
     grl_bc_query_sizes -> (the caller allocates `bytes` of device memory) -> grl_bc_begin -> grl_bc_train / grl_bc_eval ... -> grl_bc_end
   and holds nothing a checkpoint carries; the handle's own arenas are not touched except for the trained parameters and their
   entries of the gradient bucket (grl_debug_fetch "grads").  1 <= batch <= grl_config.batch_size (a larger batch is
   GRL_ERR_INVALID, the message names both numbers).  On a DQN / BDQ / auto-encoder / PPO / TRPO handle every grl_bc_* call is
   GRL_ERR_STATE before anything moves. */
typedef struct grl_bc_config {
  int32_t batch;             /* rows of a minibatch */
  float lr, adam_eps;
  const float* act_low;      /* host, [act_dim]: the action space's bounds (high > low in every dimension) */
  const float* act_high;
} grl_bc_config;
/* bytes of the session buffer: moments, scalars, loss slots, the minibatch's activations and gradients at `batch` rows, tables */
int grl_bc_query_sizes(grl_handle h, const grl_bc_config* c, size_t* bytes);
/* zeroes the buffer (the optimiser with it), builds the launch plan; synchronises.  GRL_ERR_STATE while a session is open. */
int grl_bc_begin(grl_handle h, const grl_bc_config* c, void* buf);
/* n_updates updates, back to back on the handle's stream.  obs [n_rows, obs_size] and act [n_rows, act_dim]: device, float32,
   env layout and env scale; idx [n_updates, batch]: device, int32, rows of the table -- a minibatch of fewer rows ends in -1
   entries (at least one row present).  The indices are checked on a host copy first (one synchronisation, in front of the
   updates): an index outside [-1, n_rows) or a -1 that is not trailing is GRL_ERR_INVALID naming the update and the row, and
   nothing moves.  1 <= n_updates <= 65536.  GRL_ERR_STATE without a session. */
int grl_bc_train(grl_handle h, const float* obs, const float* act, int64_t n_rows, const int32_t* idx, int n_updates);
/* forward and loss only over n_batches index rows; nothing is trained */
int grl_bc_eval(grl_handle h, const float* obs, const float* act, int64_t n_rows, const int32_t* idx, int n_batches);
/* host, synchronises: the per-update / per-batch losses of the last grl_bc_train / grl_bc_eval call; returns their number,
   GRL_ERR_INVALID when cap (in floats) is too small */
int grl_bc_get_losses(grl_handle h, float* out, int cap);
/* closes the session (synchronises): the buffer is the caller's again */
int grl_bc_end(grl_handle h);
/* Debug names while a session is open (grl_debug_fetch), of the last update / batch: "bc_obs" (the network's input: images
   [batch, 64, 64, C_img], vectors [batch, rup(obs_dim, 4)]), "bc_feat" [batch, rup(F, 4)], "bc_act" [batch, act_dim] (expert
   actions as gathered), "bc_mu", "bc_det" [batch, act_dim], "bc_dmu" [batch, rup(act_dim, 4)], "bc_loss" (the loss slots of the
   call), "bc_adam_m", "bc_adam_v" (moments over the trained range, which starts at parameter offset 0). */

/* ---- GAIL on a TRPO handle: the discriminator of stable-baselines 2.10.1 gail/adversary.py (TransitionClassifier, Box
   actions), its rewards for a rollout, and its update from the last rollout and a table of expert (observation, action) pairs.
     D(obs, act) = W3 tanh(W2 tanh(W1 [ (obs - mean) / std | act ] + b1) + b2) + b3,   two hidden layers of `hidden` units
   mean / std are those of common/mpi_running_mean_std.py with epsilon 1e-2: float64 sum (starts at 0), sumsq (1e-2) and count
   (1e-2); mean = float32(sum / count), std = sqrt(max(float32(sumsq / count) - mean^2, 1e-2)) formed in float32.
   Over generator logits g (n_g rows) and expert logits e (n_e rows), with ent(x) = (1 - sigmoid(x)) x + softplus(-x):
     total = mean softplus(g) + mean softplus(-e) - entcoeff * mean over the n_g + n_e logits of ent
   and the reward of a step is -log(1 - sigmoid(D(obs, clip(act, low, high))) + 1e-8).  The optimiser is TF-1 Adam (beta 0.9 /
   0.999) with the session's own moments and beta powers.  A session is
     grl_gail_query_sizes -> (the caller allocates `bytes` of device memory) -> grl_gail_begin -> ... -> grl_gail_end
   and lives entirely in that buffer: it holds nothing a checkpoint carries, and the handle's own arenas, plan, launch tags and
   grl_ppo_state_export bytes are what they are without it (the reward pass rewrites the rollout's reward array: that is all).
   grl_gail_begin zeroes the buffer, sets the statistics to their start values and the optimiser's words, and initialises
   NOTHING else: the caller stores the six parameter tensors (grl_gail_param_info; grl_debug_store "gail_params").
   On every handle but a TRPO handle each grl_gail_* call is GRL_ERR_STATE before anything moves; on a TRPO handle without a
   session so is every call but grl_gail_query_sizes / grl_gail_begin. */
typedef struct grl_gail_config {
  int32_t hidden;            /* hidden_size_adversary, 1 .. 1024 */
  int32_t batch;             /* generator rows of an update (and the most expert rows), 1 .. n_steps */
  float entcoeff;            /* adversary_entcoeff */
  float lr, adam_eps;        /* d_stepsize; 1e-8 */
  const float* act_low;      /* host, [act_dim]: the action space's bounds (high > low in every dimension) */
  const float* act_high;
} grl_gail_config;
int grl_gail_query_sizes(grl_handle h, const grl_gail_config* c, size_t* bytes);
/* zeroes the buffer, builds the launch plan; synchronises.  GRL_ERR_STATE while a session is open. */
int grl_gail_begin(grl_handle h, const grl_gail_config* c, void* buf);
/* tensor i of the six (TF order: adversary/fully_connected{,_1,_2}/{weights,biases}:0): its name, offset and size in floats
   inside "gail_params" (every tensor starts on a 16-byte boundary) and its shape [rows, cols]; returns 6 */
int grl_gail_param_info(grl_handle h, int i, char* name, int cap, int64_t* off, int64_t* numel, int32_t* rows, int32_t* cols);
/* Valid when all n_steps slots are closed and grl_ppo_finish has not run yet, once per rollout (GRL_ERR_STATE otherwise):
   rewrites the T stored rewards with the discriminator's in ONE batched pass over the rollout (the discriminator is fixed during
   a rollout, so this equals per-step evaluation); the environment's rewards stay readable as "gail_true_rew".  Stream-ordered,
   no synchronisation; grl_ppo_finish then forms GAE from the rewritten rewards. */
int grl_gail_rewards(grl_handle h);
/* n_updates discriminator updates, back to back on the handle's stream.  exp_obs [n_rows, obs_dim] and exp_act [n_rows,
   act_dim]: device, float32; gen_idx [n_updates, batch]: device, int32, rows of the last finished rollout, all present (their
   observations and UNCLIPPED actions are the generator's side); exp_idx [n_updates, batch]: device, int32, rows of the table --
   a shorter expert batch ends in -1 entries (at least one row present).  The indices are checked on a host copy first (one
   synchronisation, in front of the updates): GRL_ERR_INVALID names the update and the entry, and nothing moves.  Per update:
   the statistics take the gathered generator rows, then the expert rows; THEN input, forward, loss and backward at the updated
   statistics; then one Adam step.  Valid from grl_ppo_finish of a full rollout until the next grl_ppo_step writes a slot,
   whether or not grl_trpo_update ran in between (GRL_ERR_STATE otherwise).  1 <= n_updates <= 4096. */
int grl_gail_update(grl_handle h, const float* exp_obs, const float* exp_act, int64_t n_rows, const int32_t* gen_idx,
                    const int32_t* exp_idx, int n_updates);
/* host, synchronises: [n_updates, 6] of the last grl_gail_update -- generator_loss, expert_loss, entropy, entropy_loss
   (= -entcoeff * entropy), generator_acc, expert_acc (the per-block sums of the loss launch, added in index order); returns
   n_updates, GRL_ERR_INVALID when cap (in floats) is too small */
int grl_gail_get_losses(grl_handle h, float* out, int cap);
/* host, synchronise: the float64 statistics, sum / sumsq [obs_dim] and the count */
int grl_gail_get_stats(grl_handle h, double* sum, double* sumsq, double* count);
int grl_gail_set_stats(grl_handle h, const double* sum, const double* sumsq, double count);
/* closes the session (synchronises): the buffer is the caller's again */
int grl_gail_end(grl_handle h);
/* Debug names while a session is open: "gail_params", "gail_adam_m", "gail_adam_v", "gail_grads" (laid out as
   grl_gail_param_info says), "gail_x" [2 batch, rup(obs_dim + act_dim, 4)] (the last update's input: generator rows, then expert
   rows), "gail_logits" [2 batch], "gail_dlogits" [2 batch, 4] (column 0), "gail_rew_x" [T, rup(obs_dim + act_dim, 4)] and
   "gail_rew_logits" [T] (the last reward pass), "gail_true_rew" [T]. */

/* debugging / parity: copy a named internal activation of the last update to the host.
   Names: "x_obs","x_next","feat_pi","feat_vf","feat_tgt","mu","log_std","pi","logp","qf1","qf2",
   "v","v_tgt","qf1_pi","qf2_pi","rew","done".  Returns the number of floats written or <0. */
int64_t grl_debug_fetch(grl_handle h, const char* name, float* out, int64_t cap);
/* debugging / parity: overwrite the first n floats of a named internal tensor from host memory (the parity
   tests place arbitrary stored priorities "per_p" or optimiser moments "adam_m" / "adam_v" this way; no
   reference call stands behind it).  Synchronises the stream.  Returns n or <0. */
int64_t grl_debug_store(grl_handle h, const char* name, const float* in, int64_t n);

/* Checkpoint and resume (DESIGN.md "Checkpoints").  The training state lives in three places: the STATE arena
   (parameters, Adam moments, DevScalars with the beta powers / learning rate / Philox counters / replay size, the
   sample-time and running VecNormalize statistics with their double-buffered count) and the REPLAY arena (ring, priority
   leaves, block sums, PerState) -- both caller-owned, the caller copies them -- and a few host-side fields of the handle,
   which the three calls below move as one opaque blob:
     grl_state_size    bytes grl_state_export will write now (it depends on how many observations grl_observe holds);
     grl_state_export  host; synchronises the handle's stream.  Writes a grl_state_header, the grl_config the handle was
                       created with, the host fields (ring cursor and size, parity of the running-statistics double
                       buffer, rows held by grl_observe) and -- the only training state in the WORK arena -- the
                       observations of the last two grl_observe calls.  Returns the bytes written, GRL_ERR_INVALID when
                       cap is too small;
     grl_state_import  host; synchronises.  Checks everything before it changes anything: GRL_ERR_INVALID for a short or
                       foreign blob (magic, grl_version(), layout version) and for a blob of another configuration -- the
                       message names the first grl_config field that differs -- GRL_ERR_STATE on a handle connected for
                       data parallelism while an exchange is in flight (some rank has begun an exchange another has not
                       finished).  Then restores the host fields and observed rows and re-derives the device mirror of
                       the ring size (DevScalars.replay_size) from the blob, so the caller restores the state arena
                       BEFORE importing.  A blob whose header says replay_size 0 (a caller that leaves the ring out sets
                       replay_pos = replay_size = 0 in the header) also returns the priority tree to its initial state.
                       Captured graphs stay valid: they hold arena addresses and configuration constants only, every
                       counter they read lives in device memory.
   grl_replay_segments lists the arrays of the replay arena: per-transition arrays (observations, next observations,
   direct features, actions, rewards, dones -- packed RGB rows included -- and the priority leaves) as
   {byte offset, bytes per row, rows = capacity}: rows [0, grl_replay_size) are the stored ones; arrays to be saved whole
   (block sums and minima of the priority tree, PerState) as {offset, bytes, 0}.  Returns their number, < 0 when cap is
   too small.  No reference call stands behind these four: stable-baselines checkpoints hold parameters only
   (CheckpointCallback, sb_helper.py:81). */
#define GRL_STATE_MAGIC 0x534c5247u   /* "GRLS" */
#define GRL_STATE_LAYOUT 1
typedef struct grl_state_header {
  uint32_t magic;
  int32_t version;        /* grl_version() of the writer                         */
  int32_t layout;         /* GRL_STATE_LAYOUT                                    */
  int32_t config_bytes;   /* sizeof(grl_config)                                  */
  uint64_t config_hash;   /* FNV-1a over every grl_config field, in field order  */
  int64_t replay_pos;     /* ring cursor                                         */
  int64_t replay_size;    /* stored transitions                                  */
  uint64_t total_bytes;   /* of the whole blob                                   */
} grl_state_header;
typedef struct grl_segment {
  uint64_t offset;        /* bytes from the start of the replay arena            */
  uint64_t row_bytes;     /* bytes per transition; the whole array when rows = 0 */
  int64_t rows;           /* replay_capacity, or 0: save whole                   */
} grl_segment;
int grl_state_size(grl_handle h, size_t* bytes);
int64_t grl_state_export(grl_handle h, void* host_buf, size_t cap);
int grl_state_import(grl_handle h, const void* host_buf, size_t n);
int grl_replay_segments(grl_handle h, int cap, grl_segment* out);

/* Checkpoint and resume of a PPO or TRPO handle (DESIGN.md "Checkpoints of the on-policy models").  Valid on both kinds, as
   grl_ppo_step is; GRL_ERR_STATE on every other handle (the message names the call) -- and the four calls above stay
   GRL_ERR_STATE on these two.  The training state lives in the STATE arena (parameters, Adam moments, DevScalars with the beta
   powers / learning rate / Philox counter of the action draws, PpoDev with the device's slot counter, TrpoDev, and with
   normalize = 2 the float64 running statistics with their double-buffered count) and the REPLAY arena (the rollout: observations,
   actions, values, neglogps, rewards, flags, advantages, returns, last values and flags; R = n_envs * n_steps rows, saved whole)
   -- both caller-owned, the caller copies them -- and a few host-side fields of the handle, which these calls move as one blob:
     grl_ppo_state_size    bytes grl_ppo_state_export will write now (it depends on whether grl_observe holds rows);
     grl_ppo_state_export  host; synchronises the handle's stream.  Writes a grl_state_header (replay_pos = replay_size = 0;
                           config_hash covers both configuration blocks), the grl_config and the grl_ppo_config or
                           grl_trpo_config the handle was created with (field by field, no padding bytes), behind them, in
                           this order, the rollout cursor (three int32: slots written, slots closed, finished), the parity of the running-statistics double buffer,
                           the number of rows the last grl_observe normalised (0 or n_envs) and -- the only training state in
                           the WORK arena -- those rows [n_envs, rup(obs_dim, 4)] in their normalised form, which obs == NULL
                           acts on.  NOT in the blob, and not state: the raw rows of grl_observe (normalised by the launch that
                           uploads them, read by nothing later), what a step sends and returns, the permutations and
                           diagnostics of the last training call (grl_ppo_get_metrics / grl_trpo_get_metrics are read behind
                           the call they describe), and TRPO's scratch between the launches of one update (theta_old, the
                           conjugate-gradient vectors, the line-search words): an update is never interrupted.  Returns the
                           bytes written, GRL_ERR_INVALID when cap is too small;
     grl_ppo_state_import  host; synchronises.  Checks everything before it changes anything; every failure is
                           GRL_ERR_INVALID and leaves the handle exactly as it was: a short blob ("truncated"), a foreign one
                           ("wrong magic"), another grl_version() or layout version, a blob of the other kind of handle (PPO
                           into TRPO or the reverse, or one written by grl_state_export), a blob of another configuration --
                           the message names the first field that differs as grl_config.<field>, grl_ppo_config.<field> or
                           grl_trpo_config.<field> -- and host fields out of range ("damaged": a cursor outside
                           0 <= closed <= n_steps, closed <= written <= closed + 1, or more observed rows than n_envs).
                           Then restores the host fields and the observed rows and re-derives the device's slot counter
                           (PpoDev.slot) from the blob, so the caller restores the state arena BEFORE importing; a caller
                           that leaves the rollout out empties it behind the import (grl_debug_store "ppo_slots" 0, 0, 0).
                           Captured graphs stay valid, as with grl_state_import.
   No reference call stands behind these three. */
int grl_ppo_state_size(grl_handle h, size_t* bytes);
int64_t grl_ppo_state_export(grl_handle h, void* host_buf, size_t cap);
int grl_ppo_state_import(grl_handle h, const void* host_buf, size_t n);

/* wall-clock free kernel timing: enables hipEvent timing of tagged kernels in later steps */
int grl_profile_enable(grl_handle h, int on);
/* host: average ms per launch of the kernel tagged `name` since enable; "" lists tags into name_out */
int grl_profile_query(grl_handle h, const char* name, double* avg_ms, int64_t* launches);
/* host: one "tag:avg_ms:launches:flops_per_launch:bytes_per_launch:executed_flops_per_launch" line per profiled tag
   (flops = algorithmic 2*M*N*K over taps that exist; executed >= flops only for the masked backward-data form) */
int grl_profile_dump(grl_handle h, char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif /* GRL_H_ */
