/* RigidPointOptimizer::optimize_sampled -- one gsdf_track_sampled call; pose_ persists across frames
 * (constant-position motion model, RigidOptimizer.h:64). */
#include "RigidOptimizer.h"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <stdexcept>

bool RigidPointOptimizer::optimize_sampled(const DepthImage& depth, const Mat3f K, size_t sampling) {
    MapGradPixelSdf* map = dynamic_cast<MapGradPixelSdf*>(tSDF_);
    if (!map) throw std::runtime_error("RigidPointOptimizer needs a MapGradPixelSdf or a MapPixelSdf");
    int conv = 0, passes = 0;
    const int rc = gsdf_track_sampled(map->ctx_, depth.data(), K.data(), pose_.pose7(), num_iterations_, conv_threshold_,
                                      damping_, (int)std::min<size_t>(sampling, 1u << 20), &conv, &passes);
    if (rc != GSDF_OK) throw std::runtime_error(std::string("gsdf_track_sampled: ") + gsdf_last_error());
    last_passes_ = passes;
    if (conv) std::cout << "... Convergence after " << passes - 1 << " iterations!" << std::endl;   /* .cpp:89 */
    return conv != 0;
}

bool RigidPointOptimizer::optimize_points(const float* xyz, size_t n) {
    MapGradPixelSdf* map = dynamic_cast<MapGradPixelSdf*>(tSDF_);
    if (!map) throw std::runtime_error("RigidPointOptimizer needs a MapGradPixelSdf");
    int conv = 0, passes = 0;
    const int rc = loss_ == 0 ? gsdf_align_points(map->ctx_, xyz, (int64_t)n, pose_.pose7(), num_iterations_, conv_threshold_, damping_,
                                                  &conv, &passes, nullptr)
                              : gsdf_align_points_robust(map->ctx_, xyz, (int64_t)n, pose_.pose7(), num_iterations_, conv_threshold_,
                                                         damping_, loss_, loss_scale_, &conv, &passes, nullptr);
    if (rc != GSDF_OK) throw std::runtime_error(std::string("gsdf_align_points: ") + gsdf_last_error());
    last_passes_ = passes;
    if (conv) std::cout << "... Convergence after " << passes - 1 << " iterations!" << std::endl;   /* .cpp:89 */
    return conv != 0;
}

int RigidPointOptimizer::optimize_points_multi(const float* xyz, size_t n, const float* starts7, int m, int64_t min_count) {
    MapGradPixelSdf* map = dynamic_cast<MapGradPixelSdf*>(tSDF_);
    if (!map) throw std::runtime_error("RigidPointOptimizer needs a MapGradPixelSdf");
    if (!starts7 || m < 1) throw std::runtime_error("optimize_points_multi: no starting pose");
    multi_poses_.assign(starts7, starts7 + (size_t)m * 7);
    multi_converged_.assign((size_t)m, 0);
    multi_passes_.assign((size_t)m, 0);
    std::vector<float> last((size_t)m * (loss_ == 0 ? 36 : 38));
    int rc = loss_ == 0 ? gsdf_align_points_multi(map->ctx_, xyz, (int64_t)n, multi_poses_.data(), m, num_iterations_, conv_threshold_,
                                                  damping_, multi_converged_.data(), multi_passes_.data(), last.data(), nullptr)
                        : gsdf_align_points_multi_robust(map->ctx_, xyz, (int64_t)n, multi_poses_.data(), m, num_iterations_,
                                                         conv_threshold_, damping_, loss_, loss_scale_, multi_converged_.data(),
                                                         multi_passes_.data(), last.data(), nullptr);
    if (rc != GSDF_OK) throw std::runtime_error(std::string("gsdf_align_points_multi: ") + gsdf_last_error());
    int best = -1;
    rc = loss_ == 0 ? gsdf_align_best(m, multi_converged_.data(), multi_passes_.data(), last.data(), min_count, 1, &best)
                    : gsdf_align_best_robust(m, multi_converged_.data(), multi_passes_.data(), last.data(), (float)min_count, 1, &best);
    if (rc != GSDF_OK) throw std::runtime_error(std::string("gsdf_align_best: ") + gsdf_last_error());
    if (best < 0) return -1;
    pose_ = SE3::from_pose7(multi_poses_.data() + (size_t)best * 7);
    last_passes_ = multi_passes_[(size_t)best];
    std::cout << "... Start " << best << " of " << m << ": convergence after " << last_passes_ - 1 << " iterations!" << std::endl;
    return best;
}

void RigidPointOptimizer::set_loss(int loss, float scale) {
    if (loss < 0 || loss > 4) throw std::invalid_argument("RigidPointOptimizer::set_loss: loss outside 0 .. 4");
    if (loss != 0 && !(std::isfinite(scale) && scale > 0.f))
        throw std::invalid_argument("RigidPointOptimizer::set_loss: the scale must be finite and > 0");
    loss_ = loss;
    loss_scale_ = scale;
}

void RigidPointOptimizer::residuals(const float* xyz, size_t n, SE3 pose, std::vector<float>& phi, std::vector<float>& w) {
    MapGradPixelSdf* map = dynamic_cast<MapGradPixelSdf*>(tSDF_);
    if (!map) throw std::runtime_error("RigidPointOptimizer needs a MapGradPixelSdf");
    phi.assign(n, 0.f);
    w.assign(n, 0.f);
    const int rc = gsdf_align_residuals(map->ctx_, xyz, (int64_t)n, pose.pose7(), phi.data(), w.data());
    if (rc != GSDF_OK) throw std::runtime_error(std::string("gsdf_align_residuals: ") + gsdf_last_error());
}
