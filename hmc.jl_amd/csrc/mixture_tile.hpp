// mixture_tile.hpp -- the LDS tile of the predictive mixture, one copy: MIXTILE_TD draws of a slab staged per state as
// (mu, c = 1 / (sqrt 2 * sqrt(sig2))) with the weights omega = pi_end A^h of every horizon beside them, and the walk that
// evaluates the mixture CDF at a thread's point over the tile in draw order.  predictive_cdf_kernel and fan_eval_kernel are
// this tile with another source of the point; score_comp_kernel takes the transition staging and the weights and keeps its
// three-wide components and its own walk.  One expansion is why fan's Flo / Fhi and score's pit carry the bits of the CDF entry.
// The pieces are statement macros for the reason stat_device.hpp gives; profiles/r16/README.md lists
// the forms that were tried.
//
// Common parameters.  K_: the kernel's state count; p_: its parameter struct, read for nd_ld, round5 and hz[HMCG_MAXH];
// DRAW_(dd): a function-like macro, the offset of tile row dd's draw within a column, as a size_t; nv_: the tile's valid rows;
// n_h_: horizons; tid_: threadIdx.x.  Names ending in _ inside a macro are its own.
#pragma once
#include "stat_device.hpp"

namespace hmcg {

constexpr int MIXTILE_TD = 64;       // draws per LDS tile
constexpr int MIXTILE_NT = 128;      // threads per block of a kernel that stages the tile

}  // namespace hmcg

namespace hmcg_host {

// The two-wide tile in LDS: MC [TD][K][2] | Ws [TD][n_h][K] | As [K * K][TD] (with a horizon > 0).
inline size_t mixture_lds_bytes(int K, int n_h, bool with_A)
{
    return sizeof(double) * (size_t)hmcg::MIXTILE_TD * (size_t)(2 * K + n_h * K + (with_A ? K * K : 0));
}

}  // namespace hmcg_host

// ... and its three parts, declared over the block's dynamic LDS.
#define HMCG_MIX_TILE_LDS(K_, lds_, n_h_, MC_, Ws_, As_)                                                                  \
    double* MC_ = lds_;                                                                                                   \
    double* Ws_ = MC_ + MIXTILE_TD * K_ * 2;                                                                              \
    double* As_ = Ws_ + MIXTILE_TD * n_h_ * K_

// (mu, c) of the tile's draws into MC_.  score_comp_kernel stages (mu, sig2, c) with a copy to its work area and keeps its own.
#define HMCG_MIX_STAGE_MC(K_, MC_, mu_, sig2_, p_, DRAW_, nv_, tid_)                                                      \
    do {                                                                                                                  \
        for (int q_ = tid_; q_ < K_ * MIXTILE_TD; q_ += MIXTILE_NT) {                                                     \
            const int k_ = q_ / MIXTILE_TD, dd_ = q_ - k_ * MIXTILE_TD;                                                   \
            if (dd_ < nv_) {                                                                                              \
                const size_t off_ = (size_t)k_ * p_.nd_ld + DRAW_(dd_);                                                   \
                MC_[(dd_ * K_ + k_) * 2] = stat_in(mu_[off_], p_.round5);                                                 \
                MC_[(dd_ * K_ + k_) * 2 + 1] = 1.0 / (1.4142135623730951 * sqrt(stat_in(sig2_[off_], p_.round5)));        \
            }                                                                                                             \
        }                                                                                                                 \
    } while (0)

// The transition draws of the tile into As_, by column; At_ == nullptr (every horizon 0): nothing.
#define HMCG_MIX_STAGE_A(K_, As_, At_, p_, DRAW_, nv_, tid_)                                                              \
    do {                                                                                                                  \
        if (At_) {                                                                                                        \
            for (int q_ = tid_; q_ < K_ * K_ * MIXTILE_TD; q_ += MIXTILE_NT) {                                            \
                const int c_ = q_ / MIXTILE_TD, dd_ = q_ - c_ * MIXTILE_TD;                                               \
                if (dd_ < nv_) As_[q_] = stat_in(At_[(size_t)c_ * p_.nd_ld + DRAW_(dd_)], p_.round5);                     \
            }                                                                                                             \
        }                                                                                                                 \
    } while (0)

// Weights: thread (draw dd_, horizon jh_) takes pi_end through hz[jh_] products with the draw's A (staged, a barrier behind)
// and files wv_[0..K_) in Ws_.  The ladder of selects is mix_pick of mixmoments.hip, begun at 0; neither kernel takes the
// other's form.  EXTRA_: a statement run per state k_ with wv_[k_], jh_ and dd_ in scope.
#define HMCG_MIX_WEIGHTS(K_, Ws_, As_, pie_, p_, DRAW_, nv_, n_h_, tid_, EXTRA_)                                          \
    do {                                                                                                                  \
        for (int q_ = tid_; q_ < n_h_ * MIXTILE_TD; q_ += MIXTILE_NT) {                                                   \
            const int jh_ = q_ / MIXTILE_TD, dd_ = q_ - jh_ * MIXTILE_TD;                                                 \
            if (dd_ >= nv_) continue;                                                                                     \
            int h_ = 0;                                                                                                   \
            _Pragma("unroll") for (int i_ = 0; i_ < HMCG_MAXH; ++i_) h_ = jh_ == i_ ? p_.hz[i_] : h_;                     \
            double wv_[K_];                                                                                               \
            _Pragma("unroll") for (int k_ = 0; k_ < K_; ++k_) wv_[k_] = stat_in(pie_[(size_t)k_ * p_.nd_ld + DRAW_(dd_)], p_.round5); \
            for (int step_ = 0; step_ < h_; ++step_) HMCG_OMEGA_STEP(K_, wv_, As_ + dd_, MIXTILE_TD);                     \
            _Pragma("unroll") for (int k_ = 0; k_ < K_; ++k_) {                                                           \
                Ws_[(dd_ * n_h_ + jh_) * K_ + k_] = wv_[k_];                                                              \
                EXTRA_;                                                                                                   \
            }                                                                                                             \
        }                                                                                                                 \
    } while (0)

// The whole two-wide tile, ready to be walked: the stagings, the weights and the barrier behind each.
#define HMCG_MIX_TILE_STAGE(K_, MC_, Ws_, As_, mu_, sig2_, pie_, At_, p_, DRAW_, nv_, n_h_, tid_)                         \
    do {                                                                                                                  \
        HMCG_MIX_STAGE_MC(K_, MC_, mu_, sig2_, p_, DRAW_, nv_, tid_);                                                     \
        HMCG_MIX_STAGE_A(K_, As_, At_, p_, DRAW_, nv_, tid_);                                                             \
        __syncthreads();                                                                                                  \
        HMCG_MIX_WEIGHTS(K_, Ws_, As_, pie_, p_, DRAW_, nv_, n_h_, tid_, (void)0);                                        \
        __syncthreads();                                                                                                  \
    } while (0)

// The walk: acc_ += F(y_) of every draw of the tile at horizon j_, in draw order, F = sum_k w_k Phi((y - mu_k) c_k) with
// Phi = erfc(-t) / 2 and k ascending.  This is THE per-draw expression of the mixture CDF.
#define HMCG_MIX_TILE_WALK(K_, MC_, Ws_, nv_, n_h_, j_, y_, acc_)                                                         \
    do {                                                                                                                  \
        _Pragma("unroll 1") for (int dd_ = 0; dd_ < nv_; ++dd_) {                                                         \
            const double* mc_ = MC_ + dd_ * K_ * 2;                                                                       \
            const double* wj_ = Ws_ + (dd_ * n_h_ + j_) * K_;                                                             \
            double F_ = 0.0;                                                                                              \
            _Pragma("unroll") for (int k_ = 0; k_ < K_; ++k_) {                                                           \
                const double t_ = (y_ - mc_[2 * k_]) * mc_[2 * k_ + 1];                                                   \
                const double ph_ = 0.5 * erfc(-t_);                                                                       \
                F_ = k_ == 0 ? wj_[0] * ph_ : fma(wj_[k_], ph_, F_);                                                      \
            }                                                                                                             \
            acc_ += F_;                                                                                                   \
        }                                                                                                                 \
    } while (0)
