/*
 * liuzhou_hip.h -- C ABI of libliuzhou_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the self-play hot path of kuailehaha/liuzhou.  Every entry point
 * replaces one operator of the reference's PyBind11 module `v0_core`
 * (v0/src/bindings/module.cpp:874-1482) or one stage of the v1 wave loop
 * (v1/python/self_play_gpu_runner.py:159-256, v1/python/mcts_gpu.py:1249-1457); the replaced
 * reference interface is cited at each declaration (paths relative to the reference repo).
 *
 * Conventions (same for all entry points):
 *   - plain pointers + sizes, all pointers are DEVICE pointers unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - no allocation, no host synchronisation inside -> every call is hipGraph-capturable;
 *   - returns LZ_OK (0) or a negative LzStatus; on error nothing has been launched;
 *   - inputs are borrowed, outputs are caller-allocated with the documented shapes;
 *   - tensors are dense row-major; state batches use the reference's 12-tensor SoA layout
 *     (v0/include/v0/tensor_state_batch.hpp:11-35, v1/python/mcts_gpu.py:40-57).
 */
#ifndef LIUZHOU_HIP_H
#define LIUZHOU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define LZ_API
#else
#define LZ_API __attribute__((visibility("default")))
#endif

typedef enum LzStatus {
    LZ_OK = 0,
    LZ_ERR_ARG = -1,          /* null pointer / negative size / inconsistent dims */
    LZ_ERR_UNSUPPORTED = -2,  /* dims outside what the kernels are built for */
    LZ_ERR_LAUNCH = -3,       /* hipGetLastError() != hipSuccess after launch */
    LZ_ERR_ALIGN = -4,        /* pointer not aligned as documented */
    LZ_ERR_ILLEGAL = -5       /* host library only: an action is illegal for its state (the reference's CPU path raises
                                 there, fast_apply_moves.cpp:264-470; the device path is a silent no-op) */
} LzStatus;

/* Two builds export this ABI:
 *   libliuzhou_hip.so  (hipcc, gfx950): everything below, pointers are DEVICE memory, launches on `stream`;
 *   libliuzhou_host.so (g++, csrc/lz_host.cpp): the v0_core OPERATOR subset (lz_encode_actions_fast .. lz_finalize_
 *     trajectory_inplace incl. lz_root_pack_*), pointers are HOST memory, `stream` is ignored -- what the Python
 *     `v0_core` module dispatches CPU tensors to, as the reference extension does (fast_legal_mask.cpp:453).
 * The search engines, the network kernels, the RNG and the trainer / codec kernels exist in the device build only. */

/* 12-tensor state batch.  board int8[B,36] in {-1,0,1}; marks bool(uint8)[B,36]; the rest int64[B].
 * board / marks rows must be 4-byte aligned (they are for any contiguous torch tensor). */
typedef struct LzStateSoA {
    int8_t*  board;
    uint8_t* marks_black;
    uint8_t* marks_white;
    int64_t* phase;
    int64_t* current_player;
    int64_t* pending_marks_required;
    int64_t* pending_marks_remaining;
    int64_t* pending_captures_required;
    int64_t* pending_captures_remaining;
    int64_t* forced_removals_done;
    int64_t* move_count;
    int64_t* moves_since_capture;
} LzStateSoA;

LZ_API const char* lz_version(void);
LZ_API const char* lz_status_string(int status);

/* ---- rule operators ------------------------------------------------------------------------- */

/* v0_core.encode_actions_fast  (module.cpp:1294-1310; fast_legal_mask.cpp:253-418, _cuda.cu:282-485)
 * mask uint8[B,T], metadata int32[B,T,4] with T = 36+144+36+auxiliary_dim; both fully written
 * (illegal entries: mask 0, metadata -1).  placement/movement/selection dims must be 36/144/36. */
LZ_API int lz_encode_actions_fast(const LzStateSoA* states, int64_t batch,
                                  int64_t placement_dim, int64_t movement_dim,
                                  int64_t selection_dim, int64_t auxiliary_dim,
                                  uint8_t* mask, int32_t* metadata, void* stream);

/* v0_core.batch_apply_moves  (module.cpp:1311-1327; fast_apply_moves_cuda.cu:548-744)
 * child i = apply(action_codes[i], states[parent_indices[i]]).  Illegal action => child == parent
 * with the reference GPU bookkeeping (move_count bumped for every kind except placement).
 * A parent index outside [0,batch) leaves child i untouched. */
LZ_API int lz_batch_apply_moves(const LzStateSoA* states, int64_t batch,
                                const int32_t* action_codes /*[N,4]*/,
                                const int64_t* parent_indices /*[N]*/, int64_t num_actions,
                                const LzStateSoA* out /*[N]*/, void* stream);

/* in-place variant (fast_apply_moves_cuda.cu:746-917): slot_indices must be unique. */
LZ_API int lz_batch_apply_moves_inplace(const LzStateSoA* states, int64_t batch,
                                        const int32_t* action_codes /*[N,4]*/,
                                        const int64_t* slot_indices /*[N]*/, int64_t num_actions,
                                        void* stream);

/* v0_core.states_to_model_input  (module.cpp:1286-1293; v0/src/net/encoding.cpp:26-79)
 * out float32[B,11,6,6]: own, opp, own marks, opp marks, 7 phase one-hot planes. */
LZ_API int lz_states_to_model_input(const int8_t* board, const uint8_t* marks_black,
                                    const uint8_t* marks_white, const int64_t* phase,
                                    const int64_t* current_player, int64_t batch,
                                    float* out, void* stream);

/* v0_core.project_policy_logits_fast  (module.cpp:1328-1338; project_policy_logits_fast.cpp:16-164)
 * float32 heads [B,36] x3 + legal mask uint8[B,T] -> probs, masked_logits float32[B,T]. */
LZ_API int lz_project_policy_logits_fast(const float* log_p1, const float* log_p2,
                                         const float* log_pmc, const uint8_t* legal_mask,
                                         int64_t batch, int64_t placement_dim, int64_t movement_dim,
                                         int64_t selection_dim, int64_t auxiliary_dim,
                                         float* probs, float* masked_logits, void* stream);

/* ---- root search operators (variant R: v1/python/mcts_gpu.py:1249-1457) -------------------- */

/* Row compaction at the heart of v0_core.root_pack_sparse_actions (module.cpp:247-363): for every
 * row b the legal action indices are packed to the left (ascending), with their priors renormalised
 * over the row (sum clamped at 1e-8) and their action codes.  Fixed capacity `cap` (>= max legal
 * count, 80 is always enough) keeps it sync-free; the Python operator slices to the reference's
 * data-dependent [R, Amax] shapes.
 *   counts int32[B]; legal_index int32[B,cap] (-1 pad); priors float32[B,cap] (0 pad);
 *   codes int32[B,cap,4] (0 pad). */
LZ_API int lz_root_pack_rows(const uint8_t* legal_mask, const float* probs, const int32_t* metadata,
                             int64_t batch, int64_t total_dim, int64_t cap,
                             int32_t* counts, int32_t* legal_index, float* priors, int32_t* codes,
                             void* stream);

/* v0_core.root_pack_sparse_actions (module.cpp:247-363, :1357-1362) through the C ABI.  Its output shapes [R, Amax]
 * depend on the data, so it is a two-call protocol with ONE host read in between (the reference reads R and Amax back
 * too, module.cpp:295,310):
 *   1. lz_root_pack_rows (above) -> fixed-capacity rows, then
 *      lz_root_pack_plan(counts, B, rank int32[B], child_off int64[B], sizes int64[3]) -- all device memory:
 *        rank[b] = index of row b among the non-terminal rows (-1: no legal action), child_off[b] = number of legal
 *        actions in the rows before b, sizes = {R = non-terminal rows, Amax = largest count, N = sum of counts};
 *   2. the caller reads `sizes`, allocates the ten outputs and calls
 *      lz_root_pack_fill(...): terminal_mask uint8[B], valid_root_indices int64[R], counts int64[R],
 *        valid_mask uint8[R,Amax], legal_index_mat int64[R,Amax] (0 pad), priors_mat float32[R,Amax] (0 pad),
 *        action_code_mat int32[R,Amax,4] (0 pad), pack_flat_idx int64[N] (row-major positions of the valid entries),
 *        action_codes_all int32[N,4], parent_indices_all int64[N] (row b of every entry) -- the reference's 10-tuple.
 * Pointers of empty outputs (R = 0 / N = 0) may be NULL.  The int32x4 code arrays must be 16-byte aligned. */
LZ_API int lz_root_pack_plan(const int32_t* counts, int64_t batch, int32_t* rank, int64_t* child_off, int64_t* sizes,
                             void* stream);
LZ_API int lz_root_pack_fill(const int32_t* counts, const int32_t* legal_index, const float* priors,
                             const int32_t* codes, const int32_t* rank, const int64_t* child_off, int64_t batch,
                             int64_t cap, int64_t R, int64_t Amax, int64_t N, uint8_t* terminal_mask,
                             int64_t* valid_root_indices, int64_t* counts_out, uint8_t* valid_mask,
                             int64_t* legal_index_mat, float* priors_mat, int32_t* action_code_mat,
                             int64_t* pack_flat_idx, int32_t* action_codes_all, int64_t* parent_indices_all,
                             void* stream);

/* v0_core.root_puct_allocate_visits  (module.cpp:1349-1356; root_puct_fused.cu:12-117)
 * fp32 bandit: `num_simulations` serial pulls per root, lowest index wins ties.  A <= 256.
 * The one entry point of the HIP build that owns device memory: the first eager call per (device, stream) allocates
 * 16 bytes per root of scratch for the width-binned kernel (rows of <= 8 / <= 16 / <= 32 valid actions share a wave eight /
 * four / two at a time) and keeps it; a call on a capturing stream uses what exists (an eager call with the same `num_roots` first),
 * otherwise the neighbours-pair-up kernel.  Outputs do not depend on which kernel ran (bit-identical). */
LZ_API int lz_root_puct_allocate_visits(const float* priors, const float* leaf_values,
                                        const uint8_t* valid_mask, int64_t num_roots,
                                        int64_t num_actions, int64_t num_simulations,
                                        float exploration_weight, float* visits, float* value_sum,
                                        float* root_values, void* stream);
/* The same with caller-owned scratch (`workspace` >= *bytes of lz_root_puct_workspace_bytes(num_roots, &bytes) of device
 * memory, 4-byte aligned): allocation-free like every other entry point, so it can be captured on any stream -- what the fused
 * root search of liuzhou_amd/root_search_fused.py launches. */
LZ_API int lz_root_puct_workspace_bytes(int64_t num_roots, int64_t* bytes);
LZ_API int lz_root_puct_allocate_visits_ws(const float* priors, const float* leaf_values,
                                           const uint8_t* valid_mask, int64_t num_roots, int64_t num_actions,
                                           int64_t num_simulations, float exploration_weight, float* visits,
                                           float* value_sum, float* root_values, void* workspace,
                                           int64_t workspace_bytes, void* stream);

/* v0_core.root_finalize_from_visits  (module.cpp:1374-1386, :441-535) fused with the v1 sampling
 * step (mcts_gpu.py:1410-1424).  `uniforms` float32[R] in [0,1) selects sampled picks from the
 * log-space stable policy (mcts_gpu.py:853-898) by inverse CDF; NULL = argmax (sample_moves=False).
 * Outputs are fully written: policy_dense float32[B,T] (0 fill), chosen_index int64[B] (-1),
 * chosen_codes int32[B,4] (-1), chosen_valid uint8[B] (0), root_value float32[R].  M <= 256.
 * root_value[r] = sum(value_sum[r]) / max(sum(visits[r]), 1) for EVERY row; a row without a valid action (a terminal
 * root of a padded layout) keeps the fill in the other four outputs.
 * Overflow: policy = pow(max(visits, 1e-8), 1 / max(T, 1e-6)) over the valid slots, normalised (sum clamped at 1e-8), all
 * in float32 like the reference.  Once a power exceeds FLT_MAX -- at T = 0.1 from about 7132 visits on one action, at the
 * 1e-6 clamp (temperature 0) from 2 visits -- the reference's row is inf / inf = NaN on the overflowed slots and 0 on the
 * others; policy_dense keeps those NaNs (parity), and the argmax pick follows torch's max: a NaN is the maximum, the
 * first one wins, so the pick is the first overflowed action.  The sampled pick works in log space and does not overflow.
 * Preconditions: valid_root_indices in [0, B), visits finite and 0 on slots that are not valid (the reference multiplies
 * an overflowed inf by the mask's 0 there); columns of legal_index_mat outside [0, T) are not scattered. */
LZ_API int lz_root_finalize_from_visits(const int64_t* legal_index_mat, const int32_t* action_code_mat,
                                        const uint8_t* valid_mask, const float* visits,
                                        const float* value_sum, const int64_t* valid_root_indices,
                                        int64_t num_roots, int64_t max_actions, int64_t batch_size,
                                        int64_t total_action_dim, const float* root_temperatures,
                                        const float* uniforms, float* policy_dense,
                                        int64_t* chosen_index, int32_t* chosen_codes,
                                        uint8_t* chosen_valid, float* root_value, void* stream);

/* ---- self-play step operators --------------------------------------------------------------- */

/* Opening plies of a game (`opening_random_moves` of v1/python/self_play_gpu_runner.py; mcts_gpu.py:1425-1447 replaces
 * the search's pick by torch.multinomial over the uniform policy of the valid actions): for every packed row r whose root
 * valid_root_indices[r] (NULL: r itself) has force_mask[root] != 0, the chosen action becomes the k-th valid slot of the row
 * in ascending order, k = min(floor(uniforms[r] * n), n - 1), n = valid slots; chosen_valid_mask[root] = 1.  Rows without a
 * valid slot and unflagged roots are left alone; the policy target is not touched.  Run after
 * lz_root_finalize_from_visits on the same buffers. */
LZ_API int lz_root_force_uniform_picks(const int64_t* legal_index_mat, const int32_t* action_code_mat,
                                       const uint8_t* valid_mask, const int64_t* valid_root_indices, int64_t num_roots,
                                       int64_t max_actions, const uint8_t* force_mask, const float* uniforms,
                                       int64_t* chosen_action_indices, int32_t* chosen_action_codes,
                                       uint8_t* chosen_valid_mask, void* stream);

/* v0_core.self_play_step_inplace  (module.cpp:1387-1409, :632-871).  Mutates states / plies / done.
 * Per active row i it reports fin_kind[i] = 0 (game continues), 1 (ended before the move: terminal
 * root or no valid choice) or 2 (ended by the move: winner / draw / ply cap), with
 * result_from_black[i] and soft_value[i] = tanh(k*(black-white)/18). */
LZ_API int lz_self_play_step_inplace(const LzStateSoA* states, int64_t batch, int64_t* plies,
                                     uint8_t* done, const int64_t* active_idx, int64_t num_active,
                                     const int32_t* chosen_action_codes, const uint8_t* terminal_mask,
                                     const uint8_t* chosen_valid_mask, int64_t max_game_plies,
                                     float soft_value_k, int32_t* fin_kind, float* result_from_black,
                                     float* soft_value, void* stream);

/* v0_core.finalize_trajectory_inplace  (module.cpp:1410-1420, :547-630).
 * For each finished slot with step_counts > 0 writes value = sign*result, soft = sign*soft into the
 * target buffers at that game's step indices; keep[f] = step_counts[slot] > 0,
 * final_counts[f] = step_counts[slot]; counts_out int64[3] += [black wins, white wins, draws]
 * (caller zeroes counts_out). */
LZ_API int lz_finalize_trajectory_inplace(float* value_targets, float* soft_value_targets,
                                          const int8_t* player_signs, const int64_t* step_index_matrix,
                                          const int64_t* step_counts, int64_t num_games,
                                          int64_t max_steps, const int64_t* slots,
                                          const float* result_from_black,
                                          const float* soft_value_from_black, int64_t num_slots,
                                          uint8_t* keep, int64_t* final_counts, int64_t* counts_out,
                                          void* stream);


/* Fused per-ply tail of the v1 wave loop for a FIXED wave of G slots (v1/python/self_play_gpu_runner.py:205-247 with
 * v1/python/trajectory_buffer.py:63-140): finished slots stay in the batch and are masked by `done`, so that nothing
 * in the loop needs the host.  Same results as append_steps + step_index update + self_play_step_inplace +
 * finalize_trajectory_inplace on the live slots (tests/test_gpu_selfplay.py).
 *
 * lz_wave_record: live slot g (done[g]==0, ascending g) gets arena row *cursor + rank(g); its model input
 * float32[11*36], legal mask uint8[T], policy float32[T] are copied into the arena row, value / soft targets are set
 * to NaN, sign = (current_player >= 0 ? 1 : -1); step_index[g, step_counts[g]++] = row; rows[g] = row (-1 for
 * finished slots); *cursor += live count.  A row >= capacity or a full step_index row drops the sample and bumps
 * *overflow (the host sizes both so that this never happens).
 * cursor == NULL and step_index_matrix == NULL select the SLOT-MAJOR arena of the finished-row log
 * (lz_wave_log_finished): the row of slot g's step n is g * max_steps + n, capacity >= num_slots * max_steps.
 * record (optional uint8[num_slots], the playout cap's full searches): a live slot with record[g] == 0 records nothing
 * (rows[g] = -1, step_counts unchanged, no cursor advance); the recorded slots' rows stay dense.  NULL: every live slot. */
LZ_API int lz_wave_record(const uint8_t* done, int64_t num_slots, int64_t* cursor, int64_t capacity,
                          int64_t max_steps, int64_t* step_index_matrix, int64_t* step_counts, int64_t* rows,
                          int32_t* overflow, const float* model_input, const uint8_t* legal_mask,
                          const float* policy_dense, const int64_t* current_player, int64_t action_dim,
                          float* arena_state, uint8_t* arena_legal, float* arena_policy, float* arena_value,
                          float* arena_soft, int8_t* arena_sign, const uint8_t* record, void* stream);

/* lz_wave_step_finish: for every live slot apply chosen_action_codes[g] (self_play_step_inplace rules,
 * module.cpp:724-856); a game that ends has value = sign*result / soft = sign*tanh(k*delta/18) written over its rows
 * (module.cpp:547-630), outcome int64[3] += [black wins, white wins, draws] (games with >= 1 recorded step),
 * delta_hist int64[37] (optional) += final black-white piece difference clamped to [-18,18], lengths[slot_game ?
 * slot_game[g] : g] (optional) = recorded steps, *finished (optional) += 1.  reseat == 0: done[g] = 1.  reseat != 0: the slot restarts from the empty
 * board (plies, step_counts = 0, reseated[g] = 1 if given) -- the steady-state population of bench.py.
 * step_index_matrix == NULL: slot-major arena, the rows of slot g are g * max_steps + [0, step_counts[g]).
 * game_plies (optional, indexed like lengths; the playout cap, where not every search records a row): = the searches
 * the game made (plies played, + 1 when it ended at a searched terminal root), and a game is booked in outcome by
 * those, not by its recorded rows -- a game all of whose searches were fast still counts.  NULL: as above. */
LZ_API int lz_wave_step_finish(const LzStateSoA* states, int64_t num_slots, int64_t* plies, uint8_t* done,
                               const int32_t* chosen_action_codes, const uint8_t* terminal_mask,
                               const uint8_t* chosen_valid_mask, int64_t max_game_plies, float soft_value_k,
                               float* value_targets, float* soft_value_targets, const int8_t* player_signs,
                               const int64_t* step_index_matrix, int64_t* step_counts, int64_t max_steps,
                               int64_t* outcome, int64_t* delta_hist, int64_t* lengths, const int64_t* slot_game,
                               int64_t* finished, uint8_t* reseated, int reseat, int64_t* game_plies, void* stream);

/* TD(lambda) value targets from the searches' root values (off in the reference: every row gets the final result).
 * For the searched plies t = 0..L-1 of a game, Q_t = current_player_t * root_value_t (Black's frame), y_L = z (the
 * result lz_wave_step_finish books), y_t = (1 - lambda) Q_t + lambda y_{t+1}; the row recorded at ply t gets
 * value = sign * y_t.  The recurrence runs in double (as a chunked suffix scan, so not bit-equal to a sequential
 * evaluation except for lambda = 0 and 1) and every y_t is rounded to float32 once.
 *
 * lz_wave_note_value: between lz_wave_record and lz_wave_step_finish.  A live slot at ply p = plies[g] gets
 * q_hist[g, p] = current_player * root_value, hist_len[g] = p + 1, was_live[g] = 1 and, if it recorded a row this ply
 * (rows[g] >= 0, as lz_wave_record left it), step_ply[g, step_counts[g] - 1] = p; a finished slot gets was_live[g] = 0.
 * q_hist float32[num_slots, max_plies], step_ply int32[num_slots, max_plies], hist_len int32[num_slots], was_live
 * uint8[num_slots].  A ply >= max_plies writes nothing and bumps *overflow.  A re-seated slot needs no reset.
 *
 * lz_wave_td_targets: after lz_wave_step_finish (reseat == 0) and before lz_wave_log_finished.  For every slot whose
 * game ended this ply (was_live[g] && done[g]) with step_counts[g] > 0 rows: z is read back from the game's first row
 * (sign * value, exact) and value_targets[row_j] = sign[row_j] * y[step_ply[g, j]] for its rows, row_j =
 * step_index_matrix[g, j], or g * max_steps + j when step_index_matrix == NULL.  Nothing else is touched. */
LZ_API int lz_wave_note_value(const uint8_t* done, int64_t num_slots, const int64_t* plies, const int64_t* rows,
                              const int64_t* step_counts, const float* root_value, const int64_t* current_player,
                              float* q_hist, int32_t* step_ply, int32_t* hist_len, uint8_t* was_live,
                              int64_t max_plies, int32_t* overflow, void* stream);
LZ_API int lz_wave_td_targets(const uint8_t* done, const uint8_t* was_live, int64_t num_slots, double lambda,
                              const float* q_hist, const int32_t* step_ply, const int32_t* hist_len,
                              int64_t max_plies, float* value_targets, const int8_t* player_signs,
                              const int64_t* step_index_matrix, const int64_t* step_counts, int64_t max_steps,
                              void* stream);

/* Resignation with play-through calibration (v0/python/self_play_runner.py:264-266,325-374; off there by default).
 * Per live slot and searched ply, with p = plies[g], c = the side to move and v = root_value[g] (the mover's frame):
 * the ply is ELIGIBLE when the phase is movement, capture selection or counter removal, p >= min_moves and
 * terminal_mask[g] == 0; it is LOW when it is eligible and v <= threshold in float32 (a NaN is never low).
 * per_ply == 0: the mover's own counter streak[g, c > 0 ? 0 : 1] = low ? + 1 : 0, an ineligible ply clears both;
 * per_ply != 0: streak[g, 0] = low ? + 1 : 0 on every searched ply whoever moves (the reference's literal counter).
 * The slot wants to resign when the ply is low and its counter has reached `consecutive`.  Game id = (slot_game ?
 * slot_game[g] : g) + game_base plays through iff u(seed, id) < playthrough_fraction, u = one Philox draw of
 * lz_rng.h (purpose 3, ply 0, index 1023): a pure function of (seed, id), whichever slot, stream or rank seats it.
 *
 * lz_wave_resign: after lz_wave_record / lz_wave_note_value, before lz_wave_step_finish, which is then given
 * terminal_out in place of terminal_mask.  A slot at p == 0 clears its state first (a re-seated slot needs no reset).
 * A play-through game that wants to resign plays on and latches the first such event: would[g] = c (+1 / -1, 0 =
 * none), would_ply[g] = p.  Any other game that wants to resign gets resigned[g] = 1.  For every live slot
 * terminal_out[g] = terminal_mask[g] | resigned[g], was_live[g] = 1, resigned[g] = 0 / 1; a finished slot gets
 * was_live[g] = 0 and is otherwise untouched.  streak int32[num_slots, 2], would / would_ply int32[num_slots],
 * terminal_out / was_live / resigned uint8[num_slots].  threshold in [-1, 0), consecutive >= 1, min_moves >= 0,
 * playthrough_fraction in [0, 1] (LZ_ERR_ARG otherwise).
 *
 * lz_wave_resign_book: after lz_wave_step_finish (reseat == 0), before lz_wave_td_targets and lz_wave_log_finished.
 * For every slot whose game ended this ply (was_live[g] && done[g]) counters int64[8] += {resigned, resigned by
 * Black, resigned by White, play-through games finished, play-through games that wanted to resign, of those the ones
 * whose would-be resigner did not lose (false positives), plies[g] of the resigned, plies[g] - would_ply[g] of the
 * play-through games that wanted to resign}.  The result of a play-through game is formed by the step kernel's own
 * rule from terminal_out, chosen_valid_mask and the state that kernel left; no trajectory row is read. */
LZ_API int lz_wave_resign(const uint8_t* done, int64_t num_slots, const int64_t* plies, const int64_t* phase,
                          const int64_t* current_player, const float* root_value, const uint8_t* terminal_mask,
                          const int64_t* slot_game, int64_t game_base, uint64_t seed, float threshold,
                          int64_t min_moves, int32_t consecutive, float playthrough_fraction, int per_ply,
                          int32_t* streak, int32_t* would, int32_t* would_ply, uint8_t* terminal_out,
                          uint8_t* was_live, uint8_t* resigned, void* stream);
LZ_API int lz_wave_resign_book(const LzStateSoA* states, int64_t num_slots, const uint8_t* done,
                               const uint8_t* was_live, const int64_t* plies, const uint8_t* terminal_out,
                               const uint8_t* chosen_valid_mask, const uint8_t* resigned, const int32_t* would,
                               const int32_t* would_ply, const int64_t* slot_game, int64_t game_base, uint64_t seed,
                               float playthrough_fraction, int64_t* counters, void* stream);

/* Policy surprise weighting of a finished game's rows (KataGo's policySurpriseDataWeight; off in the reference).
 * Surprise of a recorded row: s = max(0, sum over legal actions with pi_a > 0 of pi_a (log pi_a - log max(p_a, 1e-30))),
 * pi = the row's policy target, p = the noise-free network prior of the searched position; double arithmetic, stored as
 * float32.  Weights of a finished game with N rows and S = sum s_j: w_j = (1 - alpha) + alpha N s_j / S if S > 1e-12 N,
 * else 1 (sum w_j = N).  Systematic resampling: u = u01 of one Philox draw of lz_rng.h (purpose 3, ply 0, index 1022), a
 * pure function of (seed, game id), game id = (slot_game ? slot_game[g] : g) + game_base; with C_j the running sum of
 * the weights in double and C_N := N, row j is written floor(C_j + u) - floor(C_(j-1) + u) times, and output slot k holds
 * source row src[k], non-decreasing in k.  The scalar arithmetic is csrc/lz_surprise.h (host and device).
 *
 * lz_wave_note_surprise: after lz_wave_record / lz_wave_note_value, before lz_wave_resign / lz_wave_step_finish.  One
 * wave per slot.  A live slot that recorded a row this ply (rows[g] >= 0) gets surprise_hist[g, step_counts[g] - 1] = s
 * from legal_mask uint8[num_slots, action_dim], policy_dense and prior float32[num_slots, action_dim]; every live slot
 * gets was_live[g] = 1, a finished one was_live[g] = 0 and is otherwise untouched.  surprise_hist float32[num_slots,
 * max_steps].  A step outside [1, max_steps] writes nothing and bumps *overflow.
 *
 * lz_wave_surprise_resample: after lz_wave_step_finish (reseat == 0), lz_wave_resign_book and lz_wave_td_targets, before
 * lz_wave_log_finished.  One wave per slot whose game ended this ply (was_live[g] && done[g]) with N = step_counts[g] >
 * 0: src[g, 0..N) is written (int32[num_slots, max_steps], scratch that stays readable) and the game's rows are
 * rewritten in place, row_k <- row_src[k] in all six arena tensors (state float32[396], legal mask uint8[action_dim],
 * policy float32[action_dim], value, soft value, sign), row_j = step_index_matrix[g, j], or g * max_steps + j when
 * step_index_matrix == NULL.  counters int64[3] += {games, their rows, rows that got no slot (= extra copies written)},
 * *surprise_sum (double) += S.  step_counts, other slots' rows and games that ended on an earlier ply are untouched.
 * action_dim must be a multiple of 4, at most 256 (LZ_ERR_UNSUPPORTED); arena_state and arena_policy 16-byte, arena_legal
 * 4-byte, surprise_sum 8-byte aligned (LZ_ERR_ALIGN); alpha in [0, 1] (LZ_ERR_ARG). */
LZ_API int lz_wave_note_surprise(const uint8_t* done, int64_t num_slots, const int64_t* rows,
                                 const int64_t* step_counts, const uint8_t* legal_mask, const float* policy_dense,
                                 const float* prior, int64_t action_dim, float* surprise_hist, uint8_t* was_live,
                                 int64_t max_steps, int32_t* overflow, void* stream);
LZ_API int lz_wave_surprise_resample(const uint8_t* done, const uint8_t* was_live, int64_t num_slots, double alpha,
                                     const float* surprise_hist, const int64_t* slot_game, int64_t game_base,
                                     uint64_t seed, float* arena_state, uint8_t* arena_legal, float* arena_policy,
                                     float* arena_value, float* arena_soft, int8_t* arena_sign, int64_t action_dim,
                                     const int64_t* step_index_matrix, const int64_t* step_counts, int64_t max_steps,
                                     int32_t* src, int64_t* counters, double* surprise_sum, void* stream);

/* lz_wave_reseat: the wave loop of self_play_gpu_runner.py:84-90 starts the next `concurrent_games` games only when the
 * whole wave has finished; here finished slots (done[g] != 0, ascending g) restart from the empty board at once while
 * *budget (games not yet started) lasts: slot_game[g] = (*next_game)++, plies / step_counts = 0, done[g] = 0,
 * reseated[g] = 1 (optional); *budget is decremented.  Deterministic (one workgroup, ordered scan).
 * logged_only != 0: a finished slot that still holds rows (step_counts[g] > 0, not yet taken by
 * lz_wave_log_finished) is not re-seated. */
LZ_API int lz_wave_reseat(const LzStateSoA* states, int64_t num_slots, uint8_t* done, int64_t* plies,
                          int64_t* step_counts, int64_t* budget, int64_t* next_game, int64_t* slot_game,
                          uint8_t* reseated, int logged_only, void* stream);

/* The start bank: self-play games that start from positions of earlier games (game forking; off in the reference, where
 * every game starts from the empty board).  The bank is a ring of packed states: entries uint8[capacity, 32] (the
 * lossless 32-byte record of csrc/lz_rules.h: four little-endian 64-bit words) and cursor int64[1] = the number of
 * positions ever appended; filled = min(*cursor, capacity), and the filled entries are the rows [0, filled).  Game id =
 * (slot_game ? slot_game[g] : g) + game_base; the draws are Philox blocks of lz_rng.h, purpose 3, pure functions of
 * (seed, id, ply).  The scalar rules are csrc/lz_start_bank.h (host and device).  counters int64[3] = {forked games,
 * sum of move_count at the fork, positions captured}.  1 <= capacity <= 2^24, probabilities in [0, 1], 0 <= min_move
 * <= max_move (LZ_ERR_ARG); entries 16-byte, cursor and counters 8-byte aligned (LZ_ERR_ALIGN).
 *
 * lz_start_bank_capture: once per ply, after lz_wave_record / lz_wave_note_value / lz_wave_note_surprise and before
 * lz_wave_resign / lz_wave_step_finish (the states are the searched roots).  Slot g is a candidate when done[g] == 0,
 * terminal_mask[g] == 0 (the search's mask), chosen_valid_mask[g] != 0, min_move <= move_count[g] <= max_move and
 * u01(draw(seed, id, plies[g], index 1020).x) < capture_prob.  In ascending slot order the candidate of rank r is
 * written to row (*cursor + r) % capacity; of more candidates than `capacity` only the last `capacity` write.  Then
 * *cursor += count and counters[2] += count.  Deterministic (one workgroup, ordered scan); capture_prob == 0 writes
 * nothing.
 *
 * lz_start_bank_seed: on the slots with fresh[g] != 0 (lz_wave_reseat's `reseated`, or the live slots before the first
 * ply).  With filled > 0, r = draw(seed, id, 0, index 1021) and u01(r.x) < fork_prob the twelve state tensors of slot g
 * become the unpacked entry (r.y * filled) >> 32 (integer arithmetic), counters[0] += 1 and counters[1] += its
 * move_count.  Nothing else of the slot is touched; the bank is only read. */
LZ_API int lz_start_bank_capture(const LzStateSoA* states, int64_t num_slots, const uint8_t* done,
                                 const uint8_t* terminal_mask, const uint8_t* chosen_valid_mask, const int64_t* plies,
                                 const int64_t* slot_game, int64_t game_base, uint64_t seed, float capture_prob,
                                 int64_t min_move, int64_t max_move, uint8_t* entries, int64_t capacity,
                                 int64_t* cursor, int64_t* counters, void* stream);
LZ_API int lz_start_bank_seed(const LzStateSoA* states, int64_t num_slots, const uint8_t* fresh,
                              const int64_t* slot_game, int64_t game_base, uint64_t seed, float fork_prob,
                              const uint8_t* entries, int64_t capacity, const int64_t* cursor, int64_t* counters,
                              void* stream);

/* The opening book: positions of a start bank as arena openings (csrc/lz_opening_book.h holds the scalar rules, host and
 * device).  Records are the 32-byte packed states of the bank, uint8[m, 32].
 *
 * lz_opening_book_keys: for record i in [0, m), one lane each, valid[i] = 1 iff the record is canonical (packing its
 * unpacked state gives the same 32 bytes), its phase is in 1..7, no cell is both black and white, the game is running
 * (game_status 0), the position has a legal action (the tree search's enumeration) and min_move <= move_count <=
 * max_move; else 0.  A valid record's keys[i] = {img0 | meta << 36, img1, img2, img3}: the four boards under the
 * symmetry sym[i] in 0..7 that makes (img0..img3) smallest (the lowest such index; lz_dedup_position_keys' choice), meta =
 * bits 50..63 of word 0 (phase, player, forced, pending marks / captures).  move_count and moves_since_capture are not
 * in the key.  An invalid record's keys[i] = {INT64_MIN | i, 0, 0, 0}, sym[i] = 0.  Every byte of valid[0..m),
 * keys[0..4m) and sym[0..m) is written, nothing else; total on any 32 bytes.  m == 0: LZ_OK without a launch.  m < 0,
 * min_move < 0 or max_move < min_move, a NULL pointer: LZ_ERR_ARG.  records, keys 16-byte aligned (LZ_ERR_ALIGN).
 *
 * lz_states_from_packed: the inverse of lz_pack_states, with a gather.  For row g in [0, n), one lane each, with j =
 * index[g] in [0, capacity) the twelve state tensors of row g become the unpacked records[j]; a row whose index is outside
 * [0, capacity) is left untouched.  Nothing else is written; records and index are only read.  For canonical records
 * lz_pack_states of the rows returns the gathered bytes.  n == 0: LZ_OK without a launch.  n < 0, capacity < 0, a NULL
 * pointer (records may be NULL when capacity == 0): LZ_ERR_ARG.  records 16-byte, index 8-byte, the three cell planes
 * 4-byte aligned (LZ_ERR_ALIGN). */
LZ_API int lz_opening_book_keys(const uint8_t* records, int64_t m, int64_t min_move, int64_t max_move, uint8_t* valid,
                                int64_t* keys, int8_t* sym, void* stream);
LZ_API int lz_states_from_packed(const uint8_t* records, int64_t capacity, const int64_t* index, int64_t n,
                                 const LzStateSoA* states, void* stream);

/* lz_wave_log_finished: finished-row log of the streaming worker.  The reference worker sees the rows of a wave only
 * after the whole wave has drained and copies them to the host with the GPU idle
 * (v1/python/self_play_worker.py:430-546: `_run_once` -> `chunk_batch.to("cpu")` -> `save_self_play_payload`); here
 * the rows of a game leave the slot-major live arena (lz_wave_record with cursor == NULL) for a game-major log the
 * moment the game has ended, so finished samples can be copied out while the wave goes on playing.
 * For every slot with done[g] != 0 and step_counts[g] > 0, in ascending slot order: its step_counts[g] rows (state
 * float32[396], legal uint8[action_dim], policy float32[action_dim], value, soft value) are appended to the log at
 * log_state[0] while they fit log_capacity, and step_counts[g] = 0; slots that do not fit wait (lz_wave_reseat with
 * logged_only does not re-seat them).  log_state int64[4] = {rows in the log, games in the log, games waiting, rows
 * waiting}; log_base int64[num_slots] is scratch.  Deterministic (one-workgroup ordered scan, then one wave per slot). */
LZ_API int lz_wave_log_finished(const uint8_t* done, int64_t* step_counts, int64_t num_slots, int64_t max_steps,
                                int64_t action_dim, const float* arena_state, const uint8_t* arena_legal,
                                const float* arena_policy, const float* arena_value, const float* arena_soft,
                                float* log_state_rows, uint8_t* log_legal, float* log_policy, float* log_value,
                                float* log_soft, int64_t log_capacity, int64_t* log_state, int64_t* log_base,
                                void* stream);

/* ---- network forward ------------------------------------------------------------------------- */

/* Packed network description (built by liuzhou_amd/net_pack.py from a ChessNet state_dict:
 * BatchNorm folded, conv weights in v_mfma_f32_16x16x32_f16 operand order).  All offsets into
 * `fparams` are in floats, `layer_offsets` (stem, conv1/conv2 per block, stacked head convs) in halfs. */
#define LZ_NET_MAX_LAYERS 96     /* stem + 2 convs per block + the stacked head convs: up to 47 residual blocks */
typedef struct LzNetDesc {
    int32_t channels;            /* trunk channels: 64 or 128 */
    int32_t blocks;              /* residual blocks (<= (LZ_NET_MAX_LAYERS - 2) / 2 = 47) */
    int32_t num_layers;          /* 2 + 2*blocks */
    int32_t max_blocks;          /* persistent grid size (0 = 256, one workgroup per CU) */
    const void* wfrag;           /* device, fp16 */
    const float* fparams;        /* device, fp32 */
    int64_t wfrag_bytes;         /* sizes of the two buffers (bounds of the kernel's buffer descriptors) */
    int64_t fparams_bytes;
    int32_t layer_offsets[LZ_NET_MAX_LAYERS];
    int32_t head_frag_offsets[4]; /* halfs: gpool_linear [64x192], fc1 [128x192], fc2 [112x128], out convs [16x64] */
    int32_t off_stem_bias, off_block0 /* a1|b1|bias1 per block, 3*C floats each */, off_trunk_a, off_trunk_b,
            off_head_bias, off_p_gwT, off_p_a2, off_p_b2, off_p_out, off_v_w1T, off_v_b1, off_v_w2T, off_v_b2;
    int32_t flags;               /* bit 0 (64 channels): 4-wave workgroups of 8 samples, two per CU (default grid 512):
                                    a half-size batch then still covers every CU -- for two half-batches evaluated
                                    concurrently on two streams;
                                    bit 1 (128 channels): 4-wave workgroups with 4 channel tiles per wave (one wave per
                                    SIMD, half the LDS operand reads; measured 2 % slower, off by default);
                                    bit 2: fp32 OPERANDS (parity mode, csrc/lz_net_f32.hip: v_mfma_f32_16x16x4_f32 on
                                    `wfrag_f32`): the reference's fp32 forward within 1e-5, at a fraction of the speed;
                                    every lz_net_forward_* entry point and the search loops honour it;
                                    bit 3: SPLIT fp16 operands (round 6, same file): every conv operand as hi + lo * 2^-11
                                    (two fp16 numbers, 22 bits), every product as three v_mfma_f32_16x16x32_f16 -- the
                                    fp32 forward within 1e-5 like bit 2, at 3/16 of its matrix-pipe time; needs `wfrag_lo` */
    const float* wfrag_f32;      /* device, fp32 conv fragments [layer][tap][K/4][Cout/16][64 lanes] at the same element
                                    offsets as `wfrag` (layer_offsets); NULL unless flags bit 2 is used */
    int64_t wfrag_f32_bytes;
    const void* wfrag_lo;        /* device, fp16: the LOW halves of the conv weights, fp16((w - fp16(w)) * 2^11), in the
                                    order and at the offsets of `wfrag` (conv layers only); NULL unless flags bit 3 is used */
    int64_t wfrag_lo_bytes;
} LzNetDesc;

/* ChessNet.forward (src/neural_network.py:213-259) + bucket_logits_to_scalar (:201-210), fused:
 * planes float32[N,11,6,6] -> log_p1 / log_p2 / log_pmc float32[N,36] (log-softmax over the board),
 * value_logits float32[N,101] (may be NULL), value float32[N] = E[bucket centre] (may be NULL).
 * fp16 MFMA operands with fp32 accumulation and an fp32 residual stream (the reference's autocast
 * inference mode, v1/python/mcts_gpu.py:640-646). */
LZ_API int lz_net_forward_f16(const LzNetDesc* net, const float* planes, int64_t batch,
                              float* log_p1, float* log_p2, float* log_pmc,
                              float* value_logits, float* value, void* stream);
/* same network, input staged directly from 32-byte packed bitboard states (lz_pack_states) instead of
 * float planes: the model-input encode (v0/src/net/encoding.cpp:26-79) is fused into the kernel's prologue */
LZ_API int lz_net_forward_packed_f16(const LzNetDesc* net, const void* packed_states, int64_t batch,
                                     float* log_p1, float* log_p2, float* log_pmc,
                                     float* value_logits, float* value, void* stream);
/* In both entry points log_p1 / log_p2 / log_pmc may all be NULL (values only: the policy head is skipped; `value`
 * is then required).  The `_counted` form takes the batch size from device memory (`*count`, clamped to `capacity`),
 * so that a producer kernel can size the batch without a host round trip (fused root search, lz_root_prepare). */
LZ_API int lz_net_forward_packed_counted_f16(const LzNetDesc* net, const void* packed_states, int64_t capacity,
                                             const int64_t* count, float* log_p1, float* log_p2, float* log_pmc,
                                             float* value_logits, float* value, void* stream);
/* Several networks of the same architecture in one launch, input from packed states.  Network k evaluates the rows
 * [align16(seg_off[k]), seg_off[k + 1]) (seg_off: device int64[num_nets + 1], read by the kernel, so a producer kernel can
 * write it; seg_off[num_nets] <= capacity): every segment starts on a 16-row boundary, so no pass of the kernel's 8 or 16
 * samples mixes two networks, and the rows between one segment's end and the next boundary are padding that no pass
 * covers (an empty segment: seg_off[k + 1] <= align16(seg_off[k])).  1 <= num_nets <= 8.  The networks must agree in
 * everything but `wfrag` and `fparams` (channels, blocks, layer / head / parameter offsets, buffer sizes, max_blocks,
 * flags bits 0-1): LZ_ERR_ARG otherwise; fp32-operand and split-fp16 networks (flags bits 2-3): LZ_ERR_UNSUPPORTED.
 * Every row's outputs are bit-identical to lz_net_forward_packed_f16 of that row with its own network. */
LZ_API int lz_net_forward_packed_multi_f16(const LzNetDesc* const* nets, int32_t num_nets, const void* packed_states,
                                           int64_t capacity, const int64_t* seg_off, float* log_p1, float* log_p2,
                                           float* log_pmc, float* value_logits, float* value, void* stream);
/* one-time kernel attribute setup (dynamic LDS size); call once per process before graph capture */
LZ_API int lz_net_configure(void);
/* sizeof(LzNetDesc) as the library was compiled: a binding that lays the struct out itself (ctypes) compares */
LZ_API int64_t lz_net_desc_bytes(void);
/* measurement aid (bench.py): when enabled every lz_net_forward_f16 launch is bracketed by HIP events on
 * its own stream; after synchronising, lz_prof_net_summary returns the summed kernel time. */
LZ_API int lz_prof_enable(int on);
LZ_API int lz_prof_net_summary(double* total_ms, int64_t* launches, int64_t* evals);
/* launches on several streams may overlap: time during which at least one bracketed launch was running */
LZ_API int lz_prof_net_busy(double* busy_ms);
/* the HBM-bound kernels of the tree search, bracketed the same way while lz_prof_enable(1): kind 0 = the fused
 * expand + backup + select kernel of one simulation (units = games), kind 1 = lz_tree_advance (units = games) */
LZ_API int lz_prof_aux_summary(int kind, double* total_ms, int64_t* launches, int64_t* units);

/* ---- device-resident tree search (variant P) --------------------------------------------------- */

/* Replaces the reference's portable full-tree search and its split-phase C++ twin:
 *   v1/python/portable_mcts.py:264-746 (PortableMCTS.search_batch) == src/mcts.py:280-548 with batch_K=1,
 *   v1/cpp/portable_mcts.cpp:448-979 (PrepareRoots / SelectLeaves / CompletePending / AdvanceRoots).
 * All buffers are caller-allocated device memory.  Per game g:
 *   nodes  [g*node_cap  .. +node_cap)   node_cap >= sims + 2 (+ the kept subtree with lz_tree_advance), <= 524288 (lz_tree_advance: four
 *                                       waves per workgroup up to 65 536 nodes, one above)
 *   path   [g*path_cap  .. +path_cap)   path_cap >= 3; a descent stops at path_cap - 1 levels (a game lasts <= 144
 *                                       plies, so 160 entries hold every reachable path)
 * Per engine: ONE edge pool `edges` of pool_chunks x edge_chunk 32-byte records, handed to the games in chunks
 * (round 4; it replaces per-game regions of (sims + 1) * 72 edges, the worst case no game ever reaches):
 *   chunk_list [g*chunk_cap .. +chunk_cap)  ids of the chunks game g owns, in the order it took them; n_chunks[g]
 *   free_chunks[pool_chunks], pool_top[1]   stack of free chunk ids and its height; the caller initialises them to
 *                                           0 .. pool_chunks-1 and pool_chunks, n_chunks / n_edges to 0
 *   pool_stats[3]   [0] += expansions refused because no chunk was free (the leaf stays unexpanded, its value is still
 *                   backed up, the next visit tries again -- results then differ from an unbounded tree, so size the
 *                   pool so that this stays 0); [1] = min(free chunks seen) (initialise to pool_chunks); [2] = fresh roots
 *                   that have not taken the chunk of their first expansion yet (initialise to 0): a chunk stays reserved
 *                   for each of them, so pool_chunks >= num_games is required
 * Every edge index in a record or hand-off array (node edge_begin, edge cbegin, path, leaf_edge) is an index into the
 * pool; (pool_chunks + 1) * edge_chunk <= 2^31.  chunk_cap * (edge_chunk - 71) >= node_cap * 72 makes the node arena the
 * only per-game bound (required by lz_tree_advance).  A kept subtree that would not leave room for the next search in
 * the NODE arena is pruned and counted (lz_tree_advance).
 * States are 32-byte packed bitboard records (lz_pack_states). */
typedef struct LzTreeDesc {
    int64_t num_games;
    int32_t node_cap, edge_chunk /* edges per chunk: power of two >= 128 */, path_cap, chunk_cap;
    double  exploration_weight;
    const void* root_state;        /* packed [B]: current game states (input of lz_tree_begin) */
    void*    nodes;                /* [B*node_cap] 48-byte records {packed state, int32 edge_begin, int32 nedges (-1 =
                                      not expanded), int32 parent node (-1 root), 4 B pad} */
    void*    edges;                /* [pool_chunks*edge_chunk] 32-byte records {double W (value sum, child mover's view),
                                      float P, uint32 N | info<<24, int32 child node or -1, int32 child edge_begin (pool
                                      index), uint8 action, uint8 child nedges, 6 B pad};
                                      info: bit0 child mover white, bit1 terminal, bits2-3 terminal value + 1 */
    int32_t* n_nodes;              /* [B] */
    int32_t* n_edges;              /* [B] next free pool index in the game's open chunk (multiple of edge_chunk: none) */
    int32_t* root_visits;          /* [B] */
    double*  root_w;               /* [B] */
    float*   root_init_value;      /* [B] */
    int32_t* path;                 /* [B*path_cap] edge index | bit 31: the mover changes from parent to child */
    int32_t* path_len;             /* [B] */
    int32_t* leaf_kind;            /* [B] 0 inactive, 1 needs evaluation, 2 terminal (value in leaf_value),
                                      3 root kept by lz_tree_advance (no evaluation, noise mix only),
                                      4 shared: a transposed twin's evaluation is reused (pos_index) */
    void*    leaf_state;           /* packed [B]: state awaiting evaluation */
    float*   leaf_value;           /* [B] */
    uint8_t* root_terminal;        /* [B] */
    const uint8_t* active;         /* [B] or NULL (all active) */
    int32_t* leaf_edge;            /* [B] edge the pending leaf hangs from (select -> expand hand-off) */
    int32_t* leaf_parent;          /* [B] node that owns that edge */
    /* Optional per-simulation trace of what the expand step consumed (parity tests of the production launch path:
     * lz_tree_search / lz_tree_search_continue under a hipGraph).  Slot 0 is the root step, slot s the s-th simulation;
     * steps beyond trace_cap are not recorded.  All NULL / 0 in production. */
    int32_t* trace_kind;           /* [trace_cap][B] leaf_kind the step saw */
    void*    trace_leaf;           /* [trace_cap][B] packed state that was evaluated */
    float*   trace_heads;          /* [trace_cap][B][108] log_p1 | log_p2 | log_pmc rows the step read (heads mode) */
    float*   trace_priors;         /* [trace_cap][B][220] softmax over the legal set before noise / renormalisation */
    float*   trace_value;          /* [trace_cap][B] evaluator value the step read */
    int64_t  trace_cap;
    int32_t* eval_count;           /* optional [B]: += 1 for every evaluation a game's expand step CONSUMED (a leaf or root it
                                    * expanded); terminal leaves, inactive slots and kept roots do not count.  NULL: off */
    int32_t* chunk_list;           /* [B*chunk_cap] */
    int32_t* n_chunks;             /* [B] */
    int32_t* free_chunks;          /* [pool_chunks] */
    int32_t* pool_top;             /* [1] */
    int32_t* pool_stats;           /* [3] */
    int64_t  pool_chunks;
    /* optional compact evaluation list of lz_tree_search / lz_tree_search_continue (all three set, live_count_cap >= sims + 2):
     * every simulation's leaves that NEED the network (live game, leaf to expand -- not a terminal leaf, not a kept
     * root) are appended to live_state (<= num_games records) and evaluated with lz_net_forward_packed_counted_f16, so a
     * launch runs ceil(live / samples-per-pass) network passes instead of one per slot: the cost of a wave that is
     * draining follows its live games (the reference's PortableMCTS.evaluate_states gets exactly the pending leaves,
     * v1/python/portable_mcts.py:337-378).  live_row[g] = row of game g's leaf in the list; live_count[s] = number
     * of leaves of simulation s.  Results are bit-identical to the dense launch.
     * Where the network has a gathering launch (lz_net_forward_packed_gather_f16) and a full launch is more network
     * passes than workgroups, the search evaluates the live leaves in place instead -- the network kernel picks them out
     * of leaf_state by their leaf_kind and writes live_count[s] itself: live_state and live_row are then UNUSED (they
     * must still be set: the scan path, env LZ_TREE_GATHER=0, the multi-network search and the parity networks use
     * them); live_count[s] holds the same numbers on both paths. */
    void*    live_state;           /* [num_games] 32-byte packed states (scan path) */
    int32_t* live_row;             /* [num_games] (scan path) */
    int64_t* live_count;           /* [live_count_cap] */
    int64_t  live_count_cap;
    /* Optional position index (all four arrays and pos_slots, or none): a leaf whose 32-byte state another node (not
     * the root) of the same tree holds is not evaluated (leaf_kind 4, shared) -- it takes that node's priors and raw
     * network value, bit for bit, and is left out of the compact lists.  Env LZ_TREE_SHARE=0 turns the look-ups off. */
    int32_t* pos_index;            /* [B*pos_slots] node index or -1 (open addressing; lz_tree_begin / lz_tree_advance reset it) */
    float*   node_value;           /* [B*node_cap] raw network value each node was expanded with */
    int32_t* leaf_src;             /* [B] source node of a shared leaf (select -> expand hand-off) */
    int32_t* share_count;          /* optional [B]: += 1 for every shared leaf a game's expand step took (NULL: off) */
    int64_t  pos_slots;            /* slots per game: a power of two >= 64 */
    /* Optional symmetric leaf evaluation (csrc/lz_symmetry.h; sym_mode 0 = off, every array unused): each evaluation of
     * game g is of sigma_k(leaf) -- leaf_state holds the transformed record, leaf_sym[g] = k -- and the expand step
     * builds the node from the true leaf, reading the heads as head[sigma_k(p)] for cell p and priors220 through the
     * action permutation.  sym_mode 1: k = sym_fixed for every evaluation; 2: k from Philox keyed by sym_seed, the
     * game's key sym_game[g], its ply sym_ply[g], a per-run salt sym_salt[g] (device memory, read at every launch: not
     * frozen into a captured graph) and the hash of the true leaf state -- the same id in every launch form.  Shared
     * leaves are not evaluated: k = 0. */
    int32_t* leaf_sym;             /* [B] */
    int32_t* trace_sym;            /* optional [trace_cap][B]: the k of every traced step (with trace_*) */
    const int32_t* sym_salt;       /* [B] (mode 2) */
    const int64_t* sym_game;       /* [B] (mode 2) */
    const int64_t* sym_ply;        /* [B] (mode 2) */
    uint64_t sym_seed;
    int32_t  sym_mode, sym_fixed;
    /* Several networks in one search (lz_tree_search_multi; unused by every other entry point): slot g belongs to
     * network g / seg_games (seg_games a multiple of 16, num_games = num_nets * seg_games).  Each simulation's compact
     * list (live_*, required) then holds network k's leaves at consecutive rows from a 16-aligned base, and
     * seg_off[s * (num_nets + 1) .. + num_nets] is that simulation's segment row of lz_net_forward_packed_multi_f16;
     * live_count[s] = the padded total. */
    int64_t  seg_games;
    int64_t* seg_off;              /* [live_count_cap * (num_nets + 1)] */
    /* Optional playout cap (lz_tree_search / lz_tree_search_continue only; NULL = off, every game runs `sims` and
     * gets the noise mix when noise is passed).  Both arrays are device memory read at every launch, so one captured
     * graph serves every ply whatever its mix of budgets.  A game with budget b expands the leaf of its simulation b and
     * selects nothing more: its tree is bit for bit the one a search with sims = b builds, and it leaves the compact
     * lists.  root_noise[g] == 0: no noise mix on game g's root (neither a fresh root nor a kept one).  The other search
     * entry points refuse a descriptor that sets either array (LZ_ERR_UNSUPPORTED). */
    const int32_t* sim_budget;     /* [B] simulations of this search per game (values above sims: sims) */
    const uint8_t* root_noise;     /* [B] 0: no root noise for game g */
    /* Optional forced playouts and policy target pruning (Wu 2019, section 3.2; 0 / NULL = off).  A game's search is
     * forced when forced_k > 0 and its root-noise switch is on (root_noise == NULL, or root_noise[g] != 0).  Select, root
     * level only: a child with N > 0 and N * N < (forced_k * P) * root_visits (in double) is due, and the descent takes the
     * due child with the lowest edge index.  lz_tree_finish_pruned takes those visits out of the training target again.
     * Honoured by lz_tree_select, lz_tree_search / _continue and lz_tree_finish_pruned; the wave, multi-network and
     * persistent searches refuse a descriptor with forced_k > 0 (LZ_ERR_UNSUPPORTED). */
    double   forced_k;
    int32_t* forced_count;         /* [B] optional: += 1 for every descent that took a due child */
    /* Optional Gumbel root search with Sequential Halving (Danihelka, Guez, Schrittwieser, Silver: "Policy improvement by
     * planning with Gumbel", ICLR 2022; gumbel_m == 0 = off).  A game's search is a Gumbel search when gumbel_m > 0 and
     * its root-noise switch is on (root_noise == NULL, or root_noise[g] != 0); such a search never mixes Dirichlet noise
     * into its root priors (the searches ignore `noise` when gumbel_m > 0).  Notation for a root with ne children in edge
     * order k: P(k) the stored prior, N(k), W(k) the edge statistics, q(k) the root mover's mean value (N > 0 only).
     *   Root step (the root expansion of lz_tree_expand(is_root) / lz_tree_search / _continue, fresh and kept roots alike):
     *     gumbel_gl[g][k]    = gumbel_g[g][k] + logf(P(k)) in fp32 (-inf where P = 0),
     *     gumbel_base[g][k]  = N0(k) = N(k) at this step, gumbel_root_base[g] = the root's own visit count at this step,
     *     gumbel_root_value[g] = v0: the network value of a root expanded in this step; for a kept root its mean value
     *                          root_w / root_visits as it stands (0 without visits).
     *   These are the only places where a transcendental function or the network touches the rule.  Everything below is
     *   double arithmetic of + - * / and comparisons on those stored bits.  Sums over the children run in ONE fixed order:
     *   lane l of 64 adds the terms of children l and l + 64 (a missing term is +0.0), then an xor butterfly over the
     *   lanes with offsets 32, 16, 8, 4, 2, 1 (x[l] = x[l] + x[l ^ offset]).
     *     Pv = sum_{N>0} P(k),  Pq = sum_{N>0} P(k) * q(k),  T = sum N(k) (integer),
     *     vmix = v0 when T == 0 or Pv <= 0, else (v0 + T * (Pq / Pv)) / (1 + T),
     *     cq(k) = q(k) for N(k) > 0, else vmix,
     *     sigma(k) = ((gumbel_c_visit + max_k N(k)) * gumbel_c_scale) * (0.5 * cq(k)),
     *     score(k) = (double)gl(k) + sigma(k).
     *   Several of these put a product next to a sum: both libraries are built with floating-point contraction off
     *   (-ffp-contract=off), and the bit-for-bit checks against a host restatement rely on it.
     *   Selection, root level only: s = root_visits - gumbel_root_base[g] (the simulations this search has started),
     *   j = min(gumbel_m, ne), cv = gumbel_table[j * gumbel_sims + min(s, gumbel_sims - 1)]; the candidates are the
     *   children with N(k) - N0(k) == cv, all children if there is none; the descent takes the candidate with the largest
     *   score, lowest edge index among equals.  No PUCT arithmetic runs on that level; deeper levels are unchanged.
     * Honoured by lz_tree_select, lz_tree_expand (root step), lz_tree_search / _continue and lz_tree_finish_gumbel; the
     * wave, multi-network and persistent searches refuse a descriptor with gumbel_m > 0 (LZ_ERR_UNSUPPORTED), and so does
     * every entry point when forced_k > 0 as well (two rules for the same level). */
    int32_t  gumbel_m;             /* considered actions m, 0..72 */
    int32_t  gumbel_sims;          /* n: row length of gumbel_table (the simulations of a search) */
    double   gumbel_c_visit, gumbel_c_scale;
    const float* gumbel_g;         /* [B][gumbel_stride] standard Gumbel variates per child rank (lz_rng_gumbel) */
    const int32_t* gumbel_table;   /* [(gumbel_m + 1)][gumbel_sims] visit count a considered child has at simulation s */
    float*   gumbel_gl;            /* [B][gumbel_stride] */
    int32_t* gumbel_base;          /* [B][gumbel_stride] */
    int32_t* gumbel_root_base;     /* [B] */
    float*   gumbel_root_value;    /* [B] */
    int32_t* gumbel_count;         /* [B] optional: += 1 for every search whose root step ran the rule */
    int64_t  gumbel_stride;        /* row stride of gumbel_g / gumbel_gl / gumbel_base, >= 72; a child at or beyond it has
                                      gl = -inf and N0 = 0 */
    /* Optional MCTS-Solver (Winands, Bjornsson, Saito 2008; solver == 0 = off: nothing below is read or written).  Exact
     * results are marked on the edges and carried up the tree as far as they decide the parent.
     *   An edge e from node X (mover mX) to a child state with mover mc is DECIDED when it is terminal (info bit 1: the game
     *   is over there, or the child has no legal move) or PROVEN (info bit 4).  Either way info bits 2..3 hold d(e) + 1 with
     *   d(e) in {-1, 0, +1} from mc's view; x(e) = d(e) if mc == mX, else -d(e) (the mover may stay the same along an edge).
     *   Node rule R(X) over X's edges: a decided edge with x = +1 -> X is proven +1; otherwise, every edge decided -> X is
     *   proven max x (0 or -1); otherwise X is undecided.
     *   Marking (the expand + backup step; the value a simulation backs up does not change, only later descents see the
     *   marks): a leaf expanded into a node X -- shared leaves included, a refused expansion not -- evaluates R(X) on the
     *   edge records it has just written; a proven X gets the proven bit and its value on its incoming edge (one atomic OR on
     *   n_info: the value bits of a non-terminal edge are 0).  That, or a leaf marked terminal -1 because it has no legal
     *   move, is a new decision on path entry j; the node that owns that edge (the root for j == 0, else the child node of
     *   path entry j - 1) is then evaluated with R, and if it is proven, path entry j - 1 -- or root_proven for j == 0 -- is
     *   marked and the climb repeats one level up.  Two dependent loads per level, only in simulations that decide something.
     *   root_proven[g]: 0 unknown, 1 lost, 2 drawn, 3 won for the root's mover.  Set from R(root) at the root step (a fresh
     *   root's expansion, a kept root's existing edges) and by the climb; lz_tree_begin and lz_tree_advance clear it.
     *   lz_tree_advance moves n_info whole: proofs survive it, also on an edge whose subtree was pruned away.
     *   Selection, on the levels PUCT decides (a root level under the forced-playout or Gumbel rule keeps that rule): a child
     *   decided with x = +1 is taken, lowest index first, without score arithmetic; otherwise the candidates are the children
     *   not decided with x = -1 (all children if there is none), scored as always but with q(k) = x(k) for a decided child at
     *   any visit count, in double, lowest index among equals.  A descent that takes a decided edge, on any level, ends there
     *   as a terminal leaf with the value of bits 2..3: it needs no evaluation and leaves the compact and gathering lists.
     *   With the solver on a search runs the one-wave step whatever the launch size (the two-waves-per-game step is not used).
     * Honoured by lz_tree_select, lz_tree_expand, lz_tree_search / _continue (dense, list and gathering launches) and
     * lz_tree_solver_pick; the wave, multi-network and persistent searches refuse a descriptor with solver != 0
     * (LZ_ERR_UNSUPPORTED). */
    int32_t  solver;               /* 0 = off */
    int32_t* root_proven;          /* [B] required when solver != 0 */
    int32_t* solver_count;         /* [B] optional: += 1 for every edge the expand step marks (proven, or terminal for want of
                                      a legal move) and every root result it sets */
    /* Optional KLD-gain early stopping (Leela Chess Zero's rule; kld_threshold == 0 = off: nothing below is read or
     * written).  Per game at the root, with the step numbering of lz_tree_search (launch s expands and backs up simulation
     * s, then selects the leaf of s + 1): n_k = the low 24 bits of root edge k's visit field now, o_k = the same value in
     * the game's row of kld_snapshot, N = sum n_k, O = sum o_k (children k = 0 .. ne - 1, ne <= 72).
     *   A game takes part in the check behind launch s when it is active (`active`), its root has edges and its budget
     *   kld_budget[g] is still > s + 1; any other game is left untouched and never counted.
     *   s == 0: the row becomes the current visits (zeros for a fresh root, the carried visits for a kept one; entries
     *   from ne on are 0).  Nothing else happens.
     *   s > 0: if O > 0 and N > O,
     *     gain = sum_{k: o_k > 0} (o_k / O) * ln(((double)o_k * N) / ((double)n_k * O))     in double;
     *   both products are exact integers below 2^53, so equal distributions give exactly 0.  Lane l of 64 adds the terms of
     *   children l and l + 64 (a missing term is +0.0), then the wave's DPP reduction adds the lanes.  The game stops iff
     *   s >= kld_min_sims and gain / (double)(N - O) < kld_threshold: kld_budget[g] = s + 1 (the leaf of s + 1 is already
     *   selected, so launch s + 1 expands it and selects nothing more: exactly what sim_budget means), kld_stops[g] += 1,
     *   kld_saved[g] += old budget - (s + 1).  kld_trace[g] = gain / (N - O) whenever a gain was formed.  In every case the
     *   row becomes the current visits.
     * lz_tree_search / lz_tree_search_continue enqueue the check behind launch 0 and behind every launch s = k *
     * kld_interval with s + 1 < sims, in the dense, list and gathering forms alike; they require sim_budget, and kld_budget
     * must alias it (LZ_ERR_ARG otherwise), so such a search runs the playout cap's kernels.  Every other search entry point
     * refuses a descriptor with kld_threshold > 0 (LZ_ERR_UNSUPPORTED), and so does every entry point when gumbel_m != 0 as
     * well (the Sequential Halving schedule is a function of a fixed budget).  kld_interval < 1, kld_min_sims < 0, a
     * negative or non-finite threshold, a NULL snapshot: LZ_ERR_ARG.  (These fields sit in front of the PUCT shape's, which
     * stay the last five of the descriptor.) */
    int32_t  kld_interval;         /* I >= 1 */
    int32_t  kld_min_sims;         /* M >= 0 */
    double   kld_threshold;        /* theta; 0 = off */
    int32_t* kld_snapshot;         /* [B][72] */
    int32_t* kld_budget;           /* [B] the writable view of sim_budget */
    int64_t* kld_stops;            /* [B] optional */
    int64_t* kld_saved;            /* [B] optional */
    double*  kld_trace;            /* [B] optional (tests); NULL in production */
    /* Optional PUCT shape: first-play urgency and a visit-scaled exploration constant (puct_shape == 0 = off: nothing below
     * is read).  Both act on the levels that PUCT decides -- a root level under the forced-playout rule and a child the solver
     * takes outright are decided before the score and stay as they are.  n_v is the visit count the level already uses:
     * root_visits at the root, the count on the incoming edge elsewhere.
     *   Bit 1, the table: c(n_v) = cpuct_table[min(n_v, cpuct_table_len - 1)] replaces exploration_weight in the score
     *   q + c * P * sqrt(max(n_v, 1)) / (1 + n), same operation order.  The host builds the table once
     *   (table[i] = c_puct + cpuct_log * ln((i + cpuct_base + 1) / cpuct_base) in float64); there is no log on the device.
     *   lz_tree_finish_pruned uses c(root_visits) wherever its rule has exploration_weight.
     *   Bit 0, first-play urgency: a child with n == 0 that the solver has not decided scores q = f instead of 0,
     *     V = W_v / n_v (one double division; W_v = root_w at the root, the incoming edge's W below it, both already in the
     *         node's mover's frame; with n_v == 0, V = (double)root_init_value),
     *     S = sum over the children with n > 0, decided or not, of (uint64)((double)P * 2^30)   (an integer sum),
     *     f = max(V - r * sqrt((double)S / 2^30), -1.0), r = fpu_root_reduction at the root and fpu_reduction below it; the
     *         product and the difference are rounded separately.
     *   Decided children keep q = x, visited children +-W / n.  fpu_reduction = 0 is a valid "on" (the parent's value).
     * A shaped level always takes the double arithmetic, and a shaped search the one-wave step at every launch size (the
     * two-waves-per-game step is not used).  Honoured by lz_tree_select, lz_tree_search / _continue (dense, list and
     * gathering launches; with the playout cap, forced playouts and the solver), lz_tree_search_multi and
     * lz_tree_finish_pruned.  With gumbel_m != 0, and in the wave and persistent searches: LZ_ERR_UNSUPPORTED.  Bit 1 with
     * a NULL table or cpuct_table_len < 2, bit 0 with a negative or non-finite reduction: LZ_ERR_ARG. */
    int32_t  puct_shape;           /* bit 0: first-play urgency, bit 1: cpuct_table; 0 = off */
    int32_t  cpuct_table_len;
    double   fpu_reduction;
    double   fpu_root_reduction;
    const double* cpuct_table;     /* [cpuct_table_len] device memory */
} LzTreeDesc;
LZ_API int64_t lz_tree_desc_bytes(void);
/* One check of the KLD-gain rule behind launch `step` (LzTreeDesc.kld_*; step 0 stores the snapshot only).  What
 * lz_tree_search enqueues between its launches, exported so that a test can drive a single check.  LZ_OK without a launch
 * when the rule is off. */
LZ_API int lz_tree_kld_check(const LzTreeDesc* tree, int64_t step, void* stream);

/* SoA batch -> packed records; packed records -> float32[B,11,6,6] model input (src/neural_network.py:15-65) */
/* Wave-batched leaves: the legacy search of src/mcts.py:280-497 (`batch_K` distinct leaves per tree and wave, no
 * virtual loss; batch_K = 1 is the protocol above).  Per-leaf arrays are slot-major [batch_k][B]; `leaf_state` is the
 * leaf of slot (j, g); the leaves that need the network are also appended to a compact list (`eval_state`, `eval_count`)
 * whose rows the network evaluates (device-counted batch) and lz_tree_wave_expand reads back through `eval_row`. */
typedef struct LzTreeWaveDesc {
    int32_t  batch_k;              /* leaves per game and wave, 1..32 */
    int32_t  path_cap;             /* entries per leaf path, > 160 (the level stack of a walk; a game lasts <= 144 plies) */
    int32_t* path;                 /* [batch_k][B][path_cap] */
    int32_t* path_len;             /* [batch_k][B] */
    int32_t* leaf_kind;            /* [batch_k][B] 0 inactive, 1 needs evaluation, 2 terminal */
    void*    leaf_state;           /* [batch_k][B] packed */
    float*   leaf_value;           /* [batch_k][B] */
    int32_t* leaf_edge;            /* [batch_k][B] */
    int32_t* leaf_parent;          /* [batch_k][B] */
    int32_t* sims_done;            /* [B] simulations used by the current search */
    int32_t* unfinished;           /* [1] games with budget left after the last lz_tree_wave_select */
    int32_t* eval_row;             /* [batch_k][B] row of the slot's leaf in the compact evaluation list */
    void*    eval_state;           /* [batch_k * B] packed: the leaves of the wave that need the network, compacted */
    int64_t* eval_count;           /* [1] length of that list (device-side batch size of the network launch) */
    int64_t* eval_total;           /* [1] sum of eval_count over the previous waves (statistics) */
    int32_t  max_backtrack_steps;  /* the reference's MAX_BACKTRACK_STEPS (src/mcts.py:337): a walk gives up after this many
                                      upward moves; every walk of a wave restarts at the root and replays the earlier
                                      ones, so the count is cumulative over the wave and the wave ends there.  0 = 128 */
    int32_t  reserved_;
} LzTreeWaveDesc;
/* SelectLeaves for a wave: up to min(batch_k, sims - sims_done) distinct leaves per game, in the order the reference
 * collects them (src/mcts.py:333-425); sims_done += leaves found.  reset_budget != 0 starts a new search. */
LZ_API int lz_tree_wave_select(const LzTreeDesc* tree, const LzTreeWaveDesc* wave, int64_t sims, int reset_budget,
                               void* stream);
/* CompletePending for a wave (src/mcts.py:427-497): terminal / no-legal-move leaves are backed up first, then the
 * evaluated leaves are expanded and backed up, each group in leaf order.  Evaluator rows (heads or priors220, values)
 * are the rows of the compact list, or slot-major [batch_k][B] when `slot_major` != 0 or priors220 is given. */
LZ_API int lz_tree_wave_expand(const LzTreeDesc* tree, const LzTreeWaveDesc* wave, const float* log_p1,
                               const float* log_p2, const float* log_pmc, const float* priors220, const float* values,
                               int slot_major, void* stream);
/* Whole search of one move in waves, enqueued from C++ (hipGraph-capturable); see lz_engine.hip. */
LZ_API int lz_tree_search_waves(const LzTreeDesc* tree, const LzTreeWaveDesc* wave, const LzNetDesc* net, int64_t sims,
                                int64_t waves, float* log_p1, float* log_p2, float* log_pmc, float* values,
                                const float* noise, int64_t noise_stride, float epsilon, int continue_trees,
                                int skip_roots, void* stream);

LZ_API int lz_pack_states(const LzStateSoA* states, int64_t batch, void* packed_out, void* stream);
LZ_API int lz_packed_to_model_input(const void* packed, int64_t batch, float* out, void* stream);

/* PrepareRoots: fresh single-node trees from root_state; the roots become the pending evaluations. */
LZ_API int lz_tree_begin(const LzTreeDesc* tree, void* stream);
/* SelectLeaves: one PUCT descent per game; leaf_kind / leaf_state / path are written. */
LZ_API int lz_tree_select(const LzTreeDesc* tree, void* stream);
/* CompletePending: expand the pending leaf of every game and back the value up (is_root: expand only,
 * optional noise float32[B,noise_stride] mixed with weight epsilon, `set_root_priors` semantics).
 * Evaluator output is either the three log-prob heads float32[B,36] (priors220 == NULL) or a dense
 * prior row float32[B,220] (injected evaluator for parity runs); values float32[B]. */
LZ_API int lz_tree_expand(const LzTreeDesc* tree, int is_root, const float* log_p1, const float* log_p2,
                          const float* log_pmc, const float* priors220, const float* values,
                          const float* noise, int64_t noise_stride, float epsilon, void* stream);
/* Root policy and move pick (portable_mcts.py:150-261, :690-727), per-child statistics (child_* are [B,out_cap]).
 *   selection policy = visits^(1/T) in log space with `temperatures`; it drives the move: sample_moves != 0:
 *     inverse-CDF sample with uniforms[g]; 0: most visits -> Q -> prior -> lowest index; force_uniform[g] != 0
 *     (opening plies): uniform over the legal children, index floor(uniforms[g] * n).
 *   policy_dense (training target) = the same with `target_temperatures` (NULL: = temperatures) on the scores
 *     visits + prior_pseudocount * normalised priors  (policy_target_temperature / _prior_pseudocount).
 * Precondition: wherever a softmax is taken (the temperature in force above 1e-6), a non-terminal root's scores have a
 *   positive sum -- at least one visited child, or prior_pseudocount > 0 for the target.  The reference raises "no policy
 *   mass" otherwise; here the row would be 0 / 0 and a sampled pick would leave chosen_index = -1 beside chosen_valid = 1,
 *   and nothing on the device checks it (no synchronisation on this path).  The host keeps it: a search runs at least one
 *   simulation (tree_engine.search_simulations refuses fewer; the playout cap and the KLD rule never lower a budget below
 *   1), every simulation ends in a visit of one root child, and a root whose expansion found no edge is terminal here.
 *   At a temperature <= 1e-6 such a root is defined: one-hot on the first maximum of the scores. */
LZ_API int lz_tree_finish(const LzTreeDesc* tree, const float* temperatures, const float* target_temperatures,
                          float prior_pseudocount, const uint8_t* force_uniform, int sample_moves,
                          const float* uniforms,
                          float* policy_dense /*[B,220]*/, int32_t* chosen_index, int32_t* chosen_code /*[B,4]*/,
                          uint8_t* chosen_valid, uint8_t* terminal_mask, float* root_value,
                          int32_t* child_count, int32_t* child_action, int32_t* child_visits,
                          float* child_prior, int64_t out_cap, void* stream);
/* lz_tree_finish with policy target pruning: for a forced game (LzTreeDesc.forced_k > 0, root-noise switch on) with a
 * non-terminal root the training target (policy_dense) is formed from the pruned visits N' instead of N:
 *   c* = the most visited child (lowest index), S* = Q(c*) + c_puct P(c*) sqrt(max(T, 1)) / (1 + N(c*)), T = root visits;
 *   every other child with N > 0: F = the smallest m with m * m >= (forced_k P) max(T, 1), L = the fewest visits at
 *   which the child's PUCT score stays below S* (N when S* - Q <= 0), N' = min(N, max(N - F, L)), N' <= 1 -> 0.
 * The selection policy, the pick, child_visits and root_value use the raw N.  child_target_visits [B,out_cap] (N'; = N
 * for games that are not forced) and pruned_visits [B] (sum of N - N') are optional.  With forced_k == 0 it writes exactly
 * what lz_tree_finish writes. */
LZ_API int lz_tree_finish_pruned(const LzTreeDesc* tree, const float* temperatures, const float* target_temperatures,
                                 float prior_pseudocount, const uint8_t* force_uniform, int sample_moves,
                                 const float* uniforms,
                                 float* policy_dense /*[B,220]*/, int32_t* chosen_index, int32_t* chosen_code /*[B,4]*/,
                                 uint8_t* chosen_valid, uint8_t* terminal_mask, float* root_value,
                                 int32_t* child_count, int32_t* child_action, int32_t* child_visits,
                                 float* child_prior, int64_t out_cap, int32_t* child_target_visits,
                                 int32_t* pruned_visits, void* stream);
/* lz_tree_finish plus the Gumbel rule (LzTreeDesc.gumbel_*).  For a game that is not a Gumbel game (gumbel_m == 0, its
 * root-noise switch off, a terminal root) it writes byte for byte what lz_tree_finish writes.  For a Gumbel game, with the
 * completed values and score(k) of LzTreeDesc formed from the statistics as they stand:
 *   pick:   L(k) = N(k) - N0(k); among the children with L(k) == max L the largest score, lowest index among equals.
 *           Temperatures, sample_moves and the pick uniform are ignored; force_uniform keeps precedence.
 *   target: policy_dense[act(k)] = softmax_k(log P(k) + sigma(k)) over all children, in double with the maximum
 *           subtracted, written as fp32; children with P = 0 get 0 (log P(k): the double logarithm of the stored prior).
 * child_visits, child_prior, root_value: raw.  gumbel_score double[B,out_cap] (the final score; 0 for other games and
 * beyond the children) and gumbel_vmix double[B] are optional. */
LZ_API int lz_tree_finish_gumbel(const LzTreeDesc* tree, const float* temperatures, const float* target_temperatures,
                                 float prior_pseudocount, const uint8_t* force_uniform, int sample_moves,
                                 const float* uniforms,
                                 float* policy_dense /*[B,220]*/, int32_t* chosen_index, int32_t* chosen_code /*[B,4]*/,
                                 uint8_t* chosen_valid, uint8_t* terminal_mask, float* root_value,
                                 int32_t* child_count, int32_t* child_action, int32_t* child_visits,
                                 float* child_prior, int64_t out_cap, double* gumbel_score, double* gumbel_vmix,
                                 void* stream);
/* MCTS-Solver pick (LzTreeDesc.solver != 0; launched after whichever lz_tree_finish* ran, same stream).  For a game with a
 * non-terminal root and force_uniform[g] == 0 (or force_uniform == NULL), with x(k) of the root's decided children:
 *   children with x = +1 exist: the pick becomes the one with the most visits, lowest edge index among equals;
 *   otherwise, if the finish picked a child decided with x = -1 and a child not so decided exists: the most visited of
 *   those, lowest edge index among equals.
 * Touches only chosen_index, chosen_code and chosen_valid; overrides [B] (optional) += 1 where the pick changed.  With
 * solver == 0 it launches nothing. */
LZ_API int lz_tree_solver_pick(const LzTreeDesc* tree, const uint8_t* force_uniform, int32_t* chosen_index,
                               int32_t* chosen_code /*[B,4]*/, uint8_t* chosen_valid, int32_t* overrides, void* stream);
/* Visit-offset / value-cutoff move pick (Leela Chess Zero's TempVisitOffset / TempValueCutoff, KataGo's chosenMoveSubtract /
 * chosenMovePrune), launched after lz_tree_finish* and before lz_tree_solver_pick on the same stream, with the arrays the
 * finish was given.  visit_offset o (finite, >= 0) and value_cutoff c (in [0, 2]); anything else is LZ_ERR_ARG.  The rule is
 * on when either is above 0; with both 0, or with sample_moves == 0, the call launches nothing and returns LZ_OK.
 * A game is re-picked only where the finish sampled its move from the visits: non-terminal root (a game that was not
 * searched counts as terminal), temperatures[g] > 1e-6, force_uniform == NULL or force_uniform[g] == 0.  For such a game,
 * with the root's children k = 0 .. ne-1 in edge order, N(k) the raw visits and q(k) the child's mean value in the root
 * mover's frame as the finish forms it (double W / N, sign from the info bit, 0 when N == 0), all in double:
 *   1. k* = the most visited child, lowest index among equals.
 *   2. n'(k) = N(k) - o.  If n'(k*) <= 0 the pick is k*.
 *   3. k is eligible if k == k*, or n'(k) > 0 and (c == 0 or q(k) >= q(k*) - c).
 *   4. w(k) = exp((log n'(k) - log n'(k*)) / T) for an eligible k != k*, w(k*) = 1, else 0;
 *      T = (double) max(temperatures[g], 1e-6f).
 *   5. C(k) = the inclusive cumulative weight in edge order, S = the total.
 *   6. the pick is the first eligible k with C(k) > (double) uniforms[g] * S, or the last eligible child if there is none.
 * uniforms[g] is the value the finish consumed: no further random number is drawn.  Only chosen_index and chosen_code
 * (index_to_code of the root's phase, as in the finish) are written, and only where the pick differs from the finish's.
 * counters int64[4] (optional), one atomic add per game and counter: [0] games the rule applied to, [1] children other than
 * k* with N > 0 and n' <= 0 (cut by the offset), [2] children other than k* with n' > 0 that failed the value test, [3] games
 * whose pick differs from the finish's.  The cumulative weights are summed by a wave scan, whose association differs from
 * a sequential sum by a few ulp of S.  One wave per game, up to 128 children; no LDS, no scratch; capturable. */
LZ_API int lz_tree_move_pick(const LzTreeDesc* tree, const float* temperatures, const uint8_t* force_uniform,
                             const float* uniforms, int sample_moves, double visit_offset, double value_cutoff,
                             int32_t* chosen_index, int32_t* chosen_code /*[B,4]*/, int64_t* counters, void* stream);
/* One whole search enqueued from C++: begin, root evaluation + expansion, then `sims` x
 * (select -> planes -> fused network -> expand + backup).  No host synchronisation; capturable. */
LZ_API int lz_tree_search(const LzTreeDesc* tree, const LzNetDesc* net, int64_t sims, float* planes /*[B,11,36]*/,
                          float* log_p1, float* log_p2, float* log_pmc, float* values, const float* noise,
                          int64_t noise_stride, float epsilon, void* stream);
/* lz_tree_search / _continue with one network per segment of seg_games slots (LzTreeDesc.seg_games / seg_off and the
 * compact lists required; 1 <= num_nets <= 8, networks as lz_net_forward_packed_multi_f16 accepts them).  One network
 * launch per simulation for all segments; no host synchronisation, capturable.  Each game's tree is what
 * lz_tree_search builds with that game's network.  Symmetric evaluation (sym_mode != 0) is refused (LZ_ERR_UNSUPPORTED);
 * the persistent kernel, waves and two-stream searches have no multi-network form. */
LZ_API int lz_tree_search_multi(const LzTreeDesc* tree, const LzNetDesc* const* nets, int32_t num_nets, int64_t sims,
                                float* log_p1, float* log_p2, float* log_pmc, float* values, const float* noise,
                                int64_t noise_stride, float epsilon, void* stream);
LZ_API int lz_tree_search_multi_continue(const LzTreeDesc* tree, const LzNetDesc* const* nets, int32_t num_nets,
                                         int64_t sims, float* log_p1, float* log_p2, float* log_pmc, float* values,
                                         const float* noise, int64_t noise_stride, float epsilon, void* stream);
/* ---- per-game counter RNG -----------------------------------------------------------------------------------
 * Replaces the library generators behind the reference's root noise and move sampling
 * (torch.distributions.Gamma / torch.multinomial on the device generator, v1/python/mcts_gpu.py:1329-1339,1410-1424;
 * torch Dirichlet in v1/python/portable_mcts.py:302-317; np.random.dirichlet in src/mcts.py:488-491), whose streams
 * depend on slot and batch composition.  Philox4x32-10 keyed by `seed`, counter = (game id, ply, purpose, index):
 * every variate is a pure function of those, so a game plays the same moves whichever slot / stream / rank runs it.
 *   lz_rng_gamma:   out[g*stride + k] = Gamma(alpha, 1) draw k of game_id[g] at ply[g], k < count (Marsaglia-Tsang);
 *                   normalised over a game's legal children these are Dirichlet(alpha) noise.
 *   lz_rng_uniform: out[g] = uniform [0,1) for `purpose` (1 = move pick, 2 = opening move, 3 = full / fast search of
 *                   the playout cap) of game_id[g] at ply[g].
 *   lz_rng_gumbel:  out[g*stride + k] = standard Gumbel draw for child rank k < count (<= 1023) of game_id[g] at ply[g]:
 *                   x = first word of the block (purpose 3, index 1 + k, attempt 0), u = ((float)(x >> 9) + 0.5f) * 2^-23,
 *                   g = -log(-log(u)) with both logarithms in double, rounded to fp32 once (an fp32 inner logarithm
 *                   would leave g with an absolute error of 6e-8 where g is close to 0).  Purpose 3 is the playout cap's, which uses index 0 only.
 * game_id NULL: g itself; ply NULL: 0. */
LZ_API int lz_rng_gamma(uint64_t seed, const int64_t* game_id, const int64_t* ply, int64_t batch, float alpha,
                        int64_t count, float* out, int64_t stride, void* stream);
LZ_API int lz_rng_uniform(uint64_t seed, const int64_t* game_id, const int64_t* ply, int64_t batch, int purpose,
                          float* out, void* stream);
LZ_API int lz_rng_gumbel(uint64_t seed, const int64_t* game_id, const int64_t* ply, int64_t batch, int64_t count,
                         float* out, int64_t stride, void* stream);
/* the uniforms u behind lz_rng_gumbel's variates (tests: they must equal a host restatement bit for bit) */
LZ_API int lz_rng_gumbel_uniform(uint64_t seed, const int64_t* game_id, const int64_t* ply, int64_t batch, int64_t count,
                                 float* out, int64_t stride, void* stream);

/* ---- fused root-PUCT search (variant R) on packed states -------------------------------------------------
 * The host chain of v1/python/mcts_gpu.py:1249-1457 (encode -> project -> root_pack -> noise -> apply -> evaluate
 * children -> perspective / terminal / soft value -> leaf matrix) as two fixed-shape kernels around the network
 * launches; afterwards lz_root_puct_allocate_visits / lz_root_finalize_from_visits run on the padded [B,72] rows
 * (valid_root_indices = 0..B-1).  No host synchronisation anywhere: the whole search is graph-capturable.
 *   lz_root_prepare: per root -- legal set (tensor semantics), masked softmax of the combined head logits, rows packed
 *     left to 72 slots (legal_index_mat int64, priors_mat renormalised, action_code_mat int32x4, valid_mask, counts,
 *     terminal_mask = no legal action), optional Dirichlet mix (noise float32[B,72], per-row normalised, weight
 *     epsilon, rows with > 1 action), leaf_mat zeroed, child states appended to child_states (packed records) with
 *     child_ref = root*72 + slot; *n_children (device uint64, reset by the call) = number of children.
 *   lz_root_collect: child values (network, child mover's view) -> leaf_mat in the parent's view; children whose
 *     game is over get tanh(k * (black - white) / 18) from the parent's side instead. */
LZ_API int lz_root_prepare(const void* root_states, int64_t batch, const float* log_p1, const float* log_p2,
                           const float* log_pmc, const float* noise, float epsilon, int64_t* legal_index_mat,
                           float* priors_mat, int32_t* action_code_mat, uint8_t* valid_mask, int32_t* counts,
                           uint8_t* terminal_mask, float* leaf_mat, void* child_states, int32_t* child_ref,
                           uint64_t* n_children, int64_t child_capacity /* records in child_states / child_ref,
                           >= 72 * batch */, int32_t* overflow /* device counter of roots dropped because the list
                           was full (0 in correct use), may be NULL */, void* stream);
LZ_API int lz_root_collect(const void* root_states, const void* child_states, const int32_t* child_ref,
                           const float* child_values, const uint64_t* n_children, int64_t capacity,
                           float soft_value_k, float* leaf_mat, void* stream);
/* Top-K lookahead of the root search (`sparse_ply` > 1: V1RootMCTS._refine_via_topk_lookahead,
 * v1/python/mcts_gpu.py:976-1046, driven from :1150-1160), as two fixed-shape stages around one more round of
 * network + lz_root_prepare + network + lz_root_collect on the batch * top_k L2 positions:
 *   lz_root_topk_children: per root the top_k VALID children by leaf value (highest first, lowest slot among equals)
 *     -> top_slot int32[batch, top_k] (-1: fewer legal actions than that) and l2_states (packed records,
 *     batch * top_k; the position after that action; an all-zero record -- phase 0, no legal action, so that
 *     lz_root_prepare gives it no children -- for the empty picks).
 *   lz_root_refine_topk: leaf_mat[b][top_slot[b][k]] = max(itself, max over the valid entries of row b*top_k + k of
 *     the L2 leaf matrix (0 when that row has no valid entry or a non-finite maximum)).
 * A picked child without a legal reply has no grandchildren: its lookahead value is 0, as for a row whose maximum is
 * not finite (the reference's reshape at mcts_gpu.py:1030 fails on a batch that holds such a child; the operator chain
 * of liuzhou_amd/mcts_gpu.py defines it this way and the two agree). */
LZ_API int lz_root_topk_children(const void* root_states, int64_t batch, const float* leaf_mat,
                                 const uint8_t* valid_mask, const int32_t* action_code_mat, int64_t top_k,
                                 int32_t* top_slot, void* l2_states, void* stream);
LZ_API int lz_root_refine_topk(int64_t batch, int64_t top_k, const int32_t* top_slot, const float* l2_leaf_mat,
                               const uint8_t* l2_valid_mask, float* leaf_mat, void* stream);

/* AdvanceRoots (src/mcts.py:577-592, portable_mcts.py:74-87, portable_mcts.cpp:739-769): after the host has
 * played `played_action[g]` (220-d index, -1: none) and refreshed root_state, promote that child to root and keep
 * its subtree (compacted in place) with its statistics.  Games with reset[g] != 0, inactive games, children that
 * were never expanded or a child state different from root_state[g] start a fresh tree instead.  The reference's tree
 * is unbounded; here a kept subtree that would leave no room for `next_sims` more simulations in the game's NODE arena
 * is PRUNED to its oldest part that fits (a prefix in expansion order -- closed under "parent of"; edges whose child fell
 * past the cut keep their statistics and are expanded afresh when visited).  Edge room is pooled per engine and does not
 * bound a single game.  `dropped` / `pruned`: device int32[1] each, may be NULL: += subtrees forgotten whole (defensive:
 * only if not even the first 64-node chunk fits) / += subtrees pruned.
 * Follow with lz_tree_search_continue (or lz_tree_expand(is_root=1) + the split-phase loop): kept roots are not
 * re-evaluated, they only get a fresh noise mix (portable_mcts.py:617-621). */
LZ_API int lz_tree_advance(const LzTreeDesc* tree, const int32_t* played_action, const uint8_t* reset,
                           int64_t next_sims, int32_t* dropped, int32_t* pruned, void* stream);
/* measurement aid (scripts/exp_advance_phases.py): when set, every later lz_tree_advance writes per game int64[8] =
 * 100 MHz ticks at its start / after the marks / after the nodes / after the edge runs, nodes before, nodes kept, 0, 0
 * (games that start a fresh tree only write the first and the fifth).  NULL (the default) switches it off. */
LZ_API int lz_debug_advance_ticks(int64_t* ticks);
/* lz_tree_search without the begin: searches the trees prepared by lz_tree_advance. */
LZ_API int lz_tree_search_continue(const LzTreeDesc* tree, const LzNetDesc* net, int64_t sims, float* planes,
                                   float* log_p1, float* log_p2, float* log_pmc, float* values, const float* noise,
                                   int64_t noise_stride, float epsilon, void* stream);

/* The same search (fresh: continue_trees = 0, or on the trees prepared by lz_tree_advance: 1) as ONE kernel launch in
 * which a workgroup owns 8 games for the whole move: per simulation one network pass on its 8 pending leaves, then the
 * expand / backup / select step of those games, with only a workgroup barrier in between -- no kernel boundary and no
 * device-wide barrier per simulation (replaces the host loop of v1/cpp/portable_mcts.cpp:483-590,832-939 /
 * v1/python/portable_cpp_mcts.py:270-282 like lz_tree_search does; identical results: the same device code runs the
 * network pass and the tree steps).  Two such workgroups share a CU, so one's tree step overlaps the other's network
 * pass.  64-channel networks in fp16 mode only: anything else returns LZ_ERR_UNSUPPORTED and the caller uses
 * lz_tree_search.
 *   cu_slots:    int32[4096] scratch (zeroed by the call) or NULL; with stagger_us > 0 the second workgroup to arrive
 *                on a CU starts stagger_us microseconds late, so that the pair alternates its phases;
 *   phase_ticks: optional int64[grid][4] = 100 MHz ticks each workgroup spent in network passes / tree steps, its
 *                arrival slot on its CU, the CU key (grid = lz_tree_search_persistent_grid(num_games)); NULL in production. */
LZ_API int lz_tree_search_persistent(const LzTreeDesc* tree, const LzNetDesc* net, int64_t sims, float* log_p1,
                                     float* log_p2, float* log_pmc, float* values, const float* noise,
                                     int64_t noise_stride, float epsilon, int continue_trees, int32_t* cu_slots,
                                     int64_t stagger_us, int64_t* phase_ticks, void* stream);
LZ_API int lz_tree_search_persistent_grid(int64_t num_games);

/* ---- training loss (the step right after the path) --------------------- */

/* Fused forward + backward of the reference's training loss (v1/python/train_bridge.py:330-375):
 *   policy: build_combined_logits -> masked_log_softmax -> batched_policy_loss (src/policy_batch.py:95-189),
 *   value : two-hot bucket cross entropy on clamp((1-alpha)*value + alpha*soft, -1, 1) (src/neural_network.py:176-198),
 *   WDL auxiliary term reported only (its weight is 0 in the reference).
 * Inputs float32: head outputs log_p1/log_p2/log_pmc [B,36], value_logits [B,101]; legal_mask uint8 [B,220];
 * policy_target [B,220]; value_target / soft_value_target [B]; policy_weight_sum = device scalar
 * sum_b (|value_b| < 1e-8 ? policy_draw_weight : 1).
 * Outputs: terms [B,4] = {KL_b, weight_b, bucket CE_b, WDL aux_b}  (loss = sum(KL*w)/(sum(w)+1e-8) + mean(CE));
 * gradients of grad_scale * loss with respect to the four head outputs (same shapes as the inputs). */
LZ_API int lz_policy_value_loss_fwd_bwd(const float* log_p1, const float* log_p2, const float* log_pmc,
                                        const float* value_logits, const uint8_t* legal_mask,
                                        const float* policy_target, const float* value_target,
                                        const float* soft_value_target, int64_t batch, float soft_label_alpha,
                                        float anti_draw_penalty, float policy_draw_weight,
                                        const float* policy_weight_sum, float grad_scale, float* terms,
                                        float* grad_log_p1, float* grad_log_p2, float* grad_log_pmc,
                                        float* grad_value_logits, void* stream);

/* The same loss with a per-row weight rw = row_weight[b] (float32 [B]): the second instantiation
 * of the same kernel.  rw multiplies the row's policy weight and its value gradient as an absolute factor;
 * policy_weight_sum (the sum of the draw weights, without rw) and B stay the denominators:
 *   terms[b] = {KL_b, draw weight_b * rw, bucket CE_b, WDL aux_b}   (KL, CE and aux do not depend on rw)
 *   policy gradients scale with grad_scale * draw weight_b * rw / (policy_weight_sum + 1e-8),
 *   grad_value_logits with (grad_scale / B) * rw.
 * A weight of 1.0f gives every byte of the unweighted entry's outputs; a weight of 0 and finite inputs give +-0 in
 * every gradient entry of the row.  Same argument checks (NULL row_weight: LZ_ERR_ARG). */
LZ_API int lz_policy_value_loss_weighted_fwd_bwd(const float* log_p1, const float* log_p2, const float* log_pmc,
                                                 const float* value_logits, const uint8_t* legal_mask,
                                                 const float* policy_target, const float* value_target,
                                                 const float* soft_value_target, const float* row_weight,
                                                 int64_t batch, float soft_label_alpha, float anti_draw_penalty,
                                                 float policy_draw_weight, const float* policy_weight_sum,
                                                 float grad_scale, float* terms, float* grad_log_p1,
                                                 float* grad_log_p2, float* grad_log_pmc, float* grad_value_logits,
                                                 void* stream);

/* The same loss with a distributional value target for some rows: two more instantiations of the
 * same kernel.  The arguments of the weighted entry, then dist_row int32 [B], value_dist float32 [D,101] (the table of
 * lz_merge_value_distributions) and D.  row_weight may be NULL: the unweighted arithmetic.  A row b with
 * 0 <= dist_row[b] < D takes row dist_row[b] of the table as its value target in place of the two-hot of its value and
 * soft value: terms[b][2] is the cross entropy against that row, grad_value_logits (softmax - row) * scale.  Any other
 * dist_row[b] takes the scalar two-hot path: every byte of the row's outputs is that of the entry without a table.
 * Policy, the weight column, the WDL term and every scale are untouched; the table was built for anti_draw_penalty 0,
 * which the callers pass.  Nothing outside the table and the row's own data is read.  NULL dist_row, D < 0 or a NULL
 * value_dist with D > 0: LZ_ERR_ARG; otherwise the checks of the entries above. */
LZ_API int lz_policy_value_loss_dist_fwd_bwd(const float* log_p1, const float* log_p2, const float* log_pmc,
                                             const float* value_logits, const uint8_t* legal_mask,
                                             const float* policy_target, const float* value_target,
                                             const float* soft_value_target, const float* row_weight,
                                             int64_t batch, float soft_label_alpha, float anti_draw_penalty,
                                             float policy_draw_weight, const float* policy_weight_sum,
                                             float grad_scale, float* terms, float* grad_log_p1,
                                             float* grad_log_p2, float* grad_log_pmc, float* grad_value_logits,
                                             void* stream, const int32_t* dist_row, const float* value_dist,
                                             int64_t D);

/* ---- compact trajectory records: wire format of the per-iteration gather ---- */

/* A row of the 5-tensor trajectory contract (v1/python/trajectory_buffer.py:11-33; 2 692 B) as an exact 360-byte
 * record: u64[4] {own | phase<<36, opp, own-marked, opp-marked}, u32[7] legal bits, f32[72] policy of the legal
 * actions in ascending index order (unused slots zero), f32 value, f32 soft value, 4 zero bytes.  unpack(pack(x))
 * reproduces every byte, with one exception: -0.0 in a plane or in the policy off the legal set compares equal to
 * zero, is packed as zero without a count and comes back as +0.0 (on a legal entry it is carried bit for bit, like
 * NaN payloads, infinities and subnormals; a non-zero legal byte comes back as 1).
 * `not_representable` (device int32, add-only) counts rows whose planes are not 0/1, whose policy is non-zero off the
 * legal set, or that have more than 72 legal actions -- never the case for self-play output; the record of such a row
 * is unspecified.  unpack is total: the phase is (w0 >> 36) & 7, bits the layout does not own are ignored, and a legal
 * bit past the 72nd gets policy 0 (nothing outside the record is read). */
#define LZ_TRAJECTORY_RECORD_BYTES 360
LZ_API int lz_pack_trajectory_rows(const float* state_tensors, const uint8_t* legal_masks,
                                   const float* policy_targets, const float* value_targets,
                                   const float* soft_value_targets, int64_t rows, void* records,
                                   int32_t* not_representable, void* stream);
LZ_API int lz_unpack_trajectory_rows(const void* records, int64_t rows, float* state_tensors, uint8_t* legal_masks,
                                     float* policy_targets, float* value_targets, float* soft_value_targets,
                                     void* stream);

/* Replay window (liuzhou_amd/replay_window.py): a training batch decoded straight out of a ring
 * of `capacity` records.  Output row j is byte for byte what lz_unpack_trajectory_rows of record slot[j] followed by
 * lz_symmetry_gather_samples with sym[j] writes (sym int8 / int32 by sym_width 1 / 4; NULL = the identity for every
 * row, sym_width then ignored); value and soft value are copied.  A slot[j] outside [0, capacity) or a sym[j] outside
 * 0..7 gives an all-zero row (planes, mask, policy, value, soft): the convention of lz_symmetry_gather_samples.
 * Unpacking is total as above: the phase is (w0 >> 36) & 7, bits the layout does not own are ignored, a legal bit past
 * the 72nd gets policy 0, nothing outside the 360 bytes of a record is read.  Policy, value and soft value are bit
 * copies (NaN payloads, -0.0 on a legal entry, infinities, subnormals).  m == 0: LZ_OK without a launch; m < 0,
 * capacity < 0, sym_width not 1 or 4 with sym != NULL, or a NULL required pointer: LZ_ERR_ARG; records 8-byte and the
 * float outputs 4-byte aligned, else LZ_ERR_ALIGN.  One wave per row; no allocation, no synchronisation, capturable.
 * HIP build only, like the codec. */
LZ_API int lz_replay_gather_rows(const void* records, int64_t capacity, const int64_t* slot /*[m]*/,
                                 const void* sym /*[m] or NULL*/, int32_t sym_width, int64_t m,
                                 float* out_planes /*[m,11,36]*/, uint8_t* out_masks /*[m,220]*/,
                                 float* out_policy /*[m,220]*/, float* out_value /*[m]*/, float* out_soft /*[m]*/,
                                 void* stream);

/* ---- board symmetries (the dihedral group D4 of the 6x6 square; csrc/lz_symmetry.h) --------------------------------
 * Element ids 0..7: identity, rotate 90 (r,c)->(c,5-r), rotate 180, rotate 270 (r,c)->(5-c,r), flip left-right
 * (r,c)->(r,5-c), flip up-down (r,c)->(5-r,c), transpose (r,c)->(c,r), anti-transpose (r,c)->(5-c,5-r).  A transformed
 * row holds at cell sigma(x) what the source held at x, and at action P_sigma(a) what it held at a (placement and
 * selection cells mapped, movement 36+4*from+d -> 36+4*sigma(from)+sigma_d(d), indices 216..219 kept).
 * `sym` is int8 (sym_width 1) or int32 (sym_width 4).  A row whose id is outside 0..7, or whose source index is
 * outside [0, n_src), is zeroed (gather_samples) or left untouched (the two transforms).  Both builds export all four entry points (the host build for CPU tensors). */

/* The tables, written to HOST memory in both builds (no launch): cells int32[8,36], actions int32[8,220],
 * inverse int32[8], compose int32[8,8] with compose[a][b] = sigma_a o sigma_b ("b first"), directions int32[8,4]. */
LZ_API int lz_symmetry_tables(int32_t* cells, int32_t* actions, int32_t* inverse, int32_t* compose, int32_t* directions);

/* Training rows: row j of each output = sigma_{sym[j]} of source row idx[j] (idx NULL: row j), in one pass over
 * planes float32[n_src,11,36] (a spatial permutation of every plane), masks uint8[n_src,220] and policy
 * float32[n_src,220] (exact bit copies).  masks / policy may be NULL together with their outputs.  One wave per row. */
LZ_API int lz_symmetry_gather_samples(const float* planes, const uint8_t* masks, const float* policy, int64_t n_src,
                                      const int64_t* idx, const void* sym, int32_t sym_width, float* out_planes,
                                      uint8_t* out_masks, float* out_policy, int64_t m, void* stream);

/* State batch: board and marks permuted, every scalar field copied.  `in` and `out` must not overlap. */
LZ_API int lz_symmetry_transform_states(const LzStateSoA* in, const void* sym, int32_t sym_width,
                                        const LzStateSoA* out, int64_t batch, void* stream);

/* Packed 32-byte records (csrc/lz_rules.h:pack): the four boards permuted, the metadata bits of word 0 above bit 35
 * kept.  The device build runs the wave function of the tree search's symmetric leaf evaluation. */
LZ_API int lz_symmetry_transform_packed(const int64_t* in /*[B,4]*/, const void* sym, int32_t sym_width,
                                        int64_t* out /*[B,4]*/, int64_t batch, void* stream);

/* ---- duplicate positions among training rows (csrc/lz_dedup.h) ---------------------------------
 * A row whose planes 0..3 hold only +-0.0 / 1.0 and whose planes 4..10 are each constant at +-0.0 / 1.0 with at most one
 * set is representable: four 36-bit boards and a phase 0..7.  Both builds export both entry points; neither allocates
 * or synchronises. */

/* Keys: keys[i] = {own' | phase<<36, opp', own_marked', opp_marked', legal bits of the image (4 words: bit b & 63 of
 * word 4 + (b >> 6))} of row i's image under sym[i] = k*: 0 when `symmetric` is 0, else the lowest element whose image
 * of the four boards is the smallest (compared word by word as unsigned numbers).  A row that is not representable
 * gets {INT64_MIN | i, 0, ..., 0}, sym 0, and adds one to *not_representable (the caller zeroes it).  planes
 * float32[n,11,36], masks uint8[n,220].  One wave per row. */
LZ_API int lz_dedup_position_keys(const float* planes, const uint8_t* masks, int64_t n, int32_t symmetric,
                                  int64_t* keys /*[n,8]*/, int8_t* sym /*[n]*/,
                                  int32_t* not_representable /*add-only*/, void* stream);

/* Merge: output row g is group g = rows order[group_begin[g] .. group_begin[g+1]) in the frame of its first member f:
 * planes and mask bit copies of row f; policy[b] = (float)(S[b] / c_p) with S[P_e(a)] += (double)policy[m][a],
 * e = sym[f]^-1 o sym[m], c_p the members whose policy has a non-zero entry (0 -> all zero); value and soft the mean
 * over all c members; out_count[g] = c.  Sums: members in order in chunks of 256, a chunk summed sequentially from 0.0,
 * the chunk sums added in order from 0.0, in double.  A group of one is a bit copy of its row.  An empty group, a
 * range outside [0, n], an `order` entry outside [0, n) or a sym outside 0..7 gives an all-zero row with count 0.
 * planes / out_planes 16-byte aligned.  One wave per group. */
LZ_API int lz_dedup_merge_groups(const float* planes, const uint8_t* masks, const float* policy,
                                 const float* value, const float* soft, int64_t n, const int8_t* sym,
                                 const int64_t* order /*[n] rows by group, ascending inside a group*/,
                                 const int64_t* group_begin /*[groups+1]*/, int64_t groups,
                                 float* out_planes, uint8_t* out_masks, float* out_policy,
                                 float* out_value, float* out_soft, int32_t* out_count, void* stream);

/* ---- duplicate positions across the replay window, record to record (csrc/lz_replay_merge.h) --
 * The same pair over 360-byte records in a ring of `capacity` records, without the 2 692-byte rows in between.  `slot`
 * int64[m] lists the selected records.  Both builds export both entry points; neither allocates or synchronises, both
 * are capturable.  Nothing outside a record's 360 bytes is read.  m == 0 (or groups == 0): LZ_OK without a launch;
 * negative sizes, `symmetric` not 0 or 1, or a NULL required pointer: LZ_ERR_ARG; records, out_records and the int64
 * arrays 8-byte, the int32 arrays 4-byte aligned, else LZ_ERR_ALIGN. */

/* Keys: keys[j] and sym[j] are byte for byte what lz_dedup_position_keys writes for the row that
 * lz_unpack_trajectory_rows makes of record slot[j] -- for any 360 bytes: the phase is (w0 >> 36) & 7, the boards are
 * masked to 36 bits, mask bits 220..223 and every bit the layout does not own are ignored.  A record is always
 * representable; a slot[j] outside [0, capacity) gives {INT64_MIN | j, 0, ..., 0}, sym 0, and adds one to
 * *not_representable (the caller zeroes it).  One wave per row; only the 88 header bytes of a record are read. */
LZ_API int lz_replay_position_keys(const void* records, int64_t capacity, const int64_t* slot /*[m]*/, int64_t m,
                                   int32_t symmetric, int64_t* keys /*[m,8]*/, int8_t* sym /*[m]*/,
                                   int32_t* not_representable /*add-only*/, void* stream);

/* Merge: `order` and `group_begin` index positions in `slot` as they index rows in lz_dedup_merge_groups, sym[m] is
 * per position.  Output record g is byte for byte lz_pack_trajectory_rows of row g of lz_dedup_merge_groups run on the
 * unpacked rows: the first member's header made canonical (boards masked, phase at bit 36 of word 0, unowned bits and
 * the pad zero, mask bits >= 220 clear); policy slot r, the first member's r-th legal action b, = (float)(S / c_p) with
 * S the sum over the members of (double) their policy at P_e^-1(b), e = sym[f]^-1 o sym[m] -- the member's slot at the
 * rank of that action among its legal bits, 0 when the bit is clear or the rank >= 72; c_p the members with a non-zero
 * entry among their first min(legal count, 72) slots (0 -> all zero); value and soft the mean over all c members; slots
 * at or past the legal count zero; out_count[g] = c.  Sums in the association of lz_dedup_merge_groups.  A group of one
 * carries its legal slots, value and soft as bit copies.  A first member with more than 72 legal bits gives the first
 * 72 legal actions' slots and adds one to *not_representable.  An empty or impossible range, an `order` entry outside
 * [0, m), a slot outside the ring or a sym outside 0..7 gives an all-zero record with count 0.  One wave per group. */
LZ_API int lz_replay_merge_records(const void* records, int64_t capacity, const int64_t* slot /*[m]*/, int64_t m,
                                   const int8_t* sym /*[m]*/, const int64_t* order /*[m]*/,
                                   const int64_t* group_begin /*[groups+1]*/, int64_t groups,
                                   void* out_records /*uint8[groups,360]*/, int32_t* out_count /*[groups]*/,
                                   int32_t* not_representable /*add-only*/, void* stream);

/* ---- the value target of a merged group as a distribution (csrc/lz_value_dist.h) -------------
 * Both merges above leave the MEAN value and soft value of a group; the bucket cross entropy of the loss is linear in
 * its target distribution, not in the value, so the lossless value target of a group is the mean of its members'
 * two-hot distributions.  Row dist_row[g] of `dist` (float32 [D,101]) receives, for group g = members
 * order[group_begin[g] .. group_begin[g+1]):
 *   dist[b] = (float)(S[b] / c),  S[b] = sum over the members, sequentially from 0.0 in member order, in double, of
 *   (double)((b == lo ? 1.0f - frac : 0) + (b == hi ? frac : 0)),
 * (lo, hi, frac) the bin assignment of lz_policy_value_loss_fwd_bwd with anti_draw_penalty 0 for the member's value and
 * soft value: mixed = fminf(fmaxf((1-alpha)*v + alpha*soft, -1), 1) uncontracted in float32 (a NaN lands on bin 0),
 * u = (mixed + 1) / (2/100), lo = floor(u) in 0..100, hi = min(lo + 1, 100), frac = clamp(u - lo, 0, 1), 0 when hi == lo.
 * A group whose members share their (value, soft) bits gets exactly that member's two-hot.
 * Member p's element is e = index[p] (index NULL: e = p); its value is the float at value_base + e * stride_bytes, its
 * soft value the float at soft_base + e * stride_bytes.  One entry serves both merges: tensors (value_base = values,
 * soft_base = soft, stride_bytes 4, index NULL, n rows) and the replay ring (value_base = ring + 348, soft_base =
 * ring + 352, stride_bytes 360, index = slot, n = capacity).
 * A group with dist_row[g] outside [0, D) writes nothing.  An `order` entry outside [0, m), an element outside [0, n)
 * or an empty or impossible range gives an all-zero row.  groups == 0 or D == 0: LZ_OK without a launch; a negative
 * size, stride_bytes < 4 or a NULL required pointer (index is optional; order only with m > 0, the bases only with
 * n > 0): LZ_ERR_ARG; the int64 arrays 8-byte, the bases, stride_bytes, dist_row and dist 4-byte aligned, else
 * LZ_ERR_ALIGN.  Both builds export it; it neither allocates nor synchronises.  One wave per group. */
LZ_API int lz_merge_value_distributions(const void* value_base, const void* soft_base, int64_t stride_bytes, int64_t n,
                                        const int64_t* index /*[m] or NULL*/, int64_t m, const int64_t* order /*[m]*/,
                                        const int64_t* group_begin /*[groups+1]*/, int64_t groups,
                                        const int32_t* dist_row /*[groups]*/, float alpha, float* dist /*[D,101]*/,
                                        int64_t D, void* stream);

/* The packed forward on the slots of a batch that are LIVE: slot g of packed_states[num_slots] is evaluated iff
 * leaf_kind[g] == 1 (device int32[num_slots]; the tree search's "leaf to expand"), and its outputs go to row g of the
 * output arrays, bit-identical to lz_net_forward_packed_f16 of that slot; rows of other slots are not written.
 * *count_out (device int64) = the number of live slots.  The launch costs ceil(live / samples-per-pass) network passes:
 * every workgroup reads the flags for itself and takes its share of the live slots in ascending order.
 * LZ_ERR_UNSUPPORTED: fp32-operand and split-fp16 networks (flags bits 2-3), or more slots than the kernel's LDS has
 * room for (12 bytes per 64 slots: about 11 000 slots for the two-per-CU 64-channel shape, which has to stay under 80 KB,
 * more than 90 000 for the others). */
LZ_API int lz_net_forward_packed_gather_f16(const LzNetDesc* net, const void* packed_states, const int32_t* leaf_kind,
                                            int64_t num_slots, int64_t* count_out, float* log_p1, float* log_p2,
                                            float* log_pmc, float* value_logits, float* value, void* stream);

/* ---- validation metrics (csrc/lz_valid.h) --------------------------------------------------------
 * Per-row metrics of the network's outputs against the targets of rows it was not trained on, and their sums by phase and
 * calibration bin.  None of the entry points allocates or synchronises; batch == 0 is LZ_OK without a launch, batch < 0
 * or a NULL pointer LZ_ERR_ARG. */

/* Rows: the inputs of lz_policy_value_loss_fwd_bwd (same shapes, same combined logits, masked log-softmax and two-hot
 * target, no anti-draw substitution) plus planes float32[batch,11,6,6], read only at cell 0 of planes 4..10.
 * rows float32[batch,12] = kl (the loss's terms[:,0]), ce, h_target, h_net (entropy of the network's policy over the
 * legal actions), top1, p_top (the network's probability of the target's best action), bucket_ce (terms[:,2]), v_hat
 * (sum of softmax(value_logits)[k] * (-1 + k / 50)), sq_err = (v_hat - z)^2, sign_ok (z not a hard draw and
 * v_hat * z > 0), decisive (z is not a hard draw: not |z| < 1e-8), policy_valid (sum of the 220 target entries > 1e-8
 * and at least one legal action).  Columns 0..5 are 0 where policy_valid is 0.
 * cls int32[batch,4] = phase (lowest k whose plane 4 + k is non-zero at cell 0, -1: none), calibration bin
 * min(9, max(0, floor((v_hat + 1) * 5))), the network's top action (-1: no legal action), the target's top action (-1
 * where policy_valid is 0).  Both arg-maxima run over the legal actions, NaN compares as -inf, ties go to the lowest
 * action.  Total: every bit pattern of every input gives defined outputs (NaN allowed).  One wave per row.  HIP build
 * only. */
LZ_API int lz_valid_row_metrics(const float* log_p1, const float* log_p2, const float* log_pmc,
                                const float* value_logits, const uint8_t* legal_mask, const float* policy_target,
                                const float* value_target, const float* soft_value_target, const float* planes,
                                int64_t batch, float soft_label_alpha, float* rows /*[batch,12]*/,
                                int32_t* cls /*[batch,4]*/, void* stream);

/* Sums: acc float64[18,14] += the batch.  Group 0 is every row, groups 1..7 the phases 0..6, groups 8..17 the calibration
 * bins 0..9 (cls columns 0 and 1; other values belong to group 0 only).  Columns 0..11 are the sums of the row columns,
 * column 12 the rows counted, column 13 the rows skipped: a row with a non-finite entry among its 12 floats is skipped in
 * each of its groups.  Association: lane l of 64 adds its rows l, l + 64, ... in order from 0.0, the 64 partial sums are
 * combined by a butterfly (distance 32, 16, ..., 1), the total is added to acc; all double, identical in both builds.
 * value float32[batch] and zsum float64[18] are optional, both or neither (LZ_ERR_ARG otherwise): zsum[g] += the value
 * targets of the rows counted in group g, by the same association (the mean z of the calibration table).
 * One wave per group; calls accumulate in stream order. */
LZ_API int lz_valid_reduce(const float* rows /*[batch,12]*/, const int32_t* cls /*[batch,4]*/,
                           const float* value /*[batch] or NULL*/, int64_t batch, double* acc /*[18,14]*/,
                           double* zsum /*[18] or NULL*/, void* stream);

/* Classification alone: phase_bin int32[batch,2] = {phase of planes float32[batch,11,6,6], calibration bin of
 * v_hat[i * v_hat_stride]} by the rules above (v_hat_stride >= 1, in floats: 12 for column 7 of a rows array).  Meant for
 * CPU arrays (the host build); the device build exports it because both libraries carry every declared symbol, and
 * lz_valid_row_metrics writes the same two values itself. */
LZ_API int lz_valid_classify(const float* planes, const float* v_hat, int64_t v_hat_stride, int64_t batch,
                             int32_t* phase_bin /*[batch,2]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIUZHOU_HIP_H */
