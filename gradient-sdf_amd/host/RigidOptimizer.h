/* RigidOptimizer / RigidPointOptimizer -- the 6-DoF point-to-SDF tracker interface of the
 * reference (cpp/include/sdf_tracker/RigidOptimizer.h:51-112, RigidPointOptimizer.h:46-73). */
#ifndef GSDF_HOST_RIGID_OPTIMIZER_H_
#define GSDF_HOST_RIGID_OPTIMIZER_H_

#include "MapGradPixelSdf.h"

#include <cstdint>
#include <vector>

class RigidOptimizer {
protected:
    int num_iterations_;
    float conv_threshold_;
    float damping_;
    Sdf* tSDF_;                                  /* non-owning, RigidOptimizer.h:62 */
    SE3 pose_ = SE3();                           /* RigidOptimizer.h:64 */
public:
    RigidOptimizer(Sdf* tSDF) : num_iterations_(25), conv_threshold_(1e-3f), damping_(1.f), tSDF_(tSDF) {}   /* :70-76 */
    RigidOptimizer(int num_iterations, float conv_threshold, float damping, Sdf* tSDF)
        : num_iterations_(num_iterations), conv_threshold_(conv_threshold), damping_(damping), tSDF_(tSDF) {}
    virtual ~RigidOptimizer() {}
    void set_num_iterations(int n) { num_iterations_ = n; }            /* :85-97 */
    void set_conv_threshold(float c) { conv_threshold_ = c; }
    void set_damping(float d) { damping_ = d; }
    int num_iterations() const { return num_iterations_; }
    float conv_threshold() const { return conv_threshold_; }
    float damping() const { return damping_; }
    void set_pose(SE3 pose) { pose_ = pose; }                          /* :99 */
    SE3 pose() { return pose_; }                                       /* :101-103 */
    virtual bool optimize(const DepthImage& depth, const Mat3f K) = 0; /* :106 */
};

class RigidPointOptimizer : public RigidOptimizer {
    int last_passes_ = 0;
    std::vector<int> multi_converged_, multi_passes_;
    std::vector<float> multi_poses_;
    int loss_ = 0;                               /* L2: the plain entries */
    float loss_scale_ = 0.f;
public:
    RigidPointOptimizer(Sdf* tSDF) : RigidOptimizer(tSDF) {}
    RigidPointOptimizer(int num_iterations, float conv_threshold, float damping, Sdf* tSDF)
        : RigidOptimizer(num_iterations, conv_threshold, damping, tSDF) {}
    /* optimize_sampled(depth, K, sampling) -- RigidPointOptimizer.h:65, .cpp:40-99 (sampling = pixel stride, .cpp:62) */
    bool optimize_sampled(const DepthImage& depth, const Mat3f K, size_t sampling);
    /* optimize() -> optimize_sampled(depth, K, 1) -- RigidPointOptimizer.h:69-72 */
    bool optimize(const DepthImage& depth, const Mat3f K) override { return optimize_sampled(depth, K, 1); }
    /* The same Gauss-Newton loop (.cpp:51-96) over n points x y z the caller brings instead of the pixels of :62-69
     * (gsdf_align_points): pose_ is the start (source -> map) and receives the result; num_iterations_, conv_threshold_ and
     * damping_ as in optimize().  A MapPixelSdf is refused (std::runtime_error). */
    bool optimize_points(const float* xyz, size_t n);
    /* optimize_points from each of the m starting poses starts7 (m x 7, e.g. gsdf_align_starts) at once
     * (gsdf_align_points_multi), then the pick of gsdf_align_best among the converged runs that hit at least min_count points.
     * Returns the picked index and sets pose_ / last_passes() to that run's, or returns -1 and leaves both alone. */
    int optimize_points_multi(const float* xyz, size_t n, const float* starts7, int m, int64_t min_count);
    /* what the last optimize_points_multi call left per start: converged flags, pass counts, poses (m x 7) */
    const std::vector<int>& multi_converged() const { return multi_converged_; }
    const std::vector<int>& multi_passes() const { return multi_passes_; }
    const std::vector<float>& multi_poses() const { return multi_poses_; }
    int last_passes() const { return last_passes_; }
    /* The loss of optimize_points / optimize_points_multi: 0 L2 (the default: the plain gsdf_align_points entries), 1 CAUCHY,
     * 2 HUBER, 3 TUKEY, 4 TRUNC_L2 (ps_optimizer/loss.h:41-48) at `scale` metres -- gsdf_align_points_robust, and for the multi
     * call the pick of gsdf_align_best_robust, where min_count is the floor of the weight sum.  A loss outside 0..4, or a scale
     * that is not finite and > 0 with a loss other than L2, throws std::invalid_argument and changes nothing.  optimize() and
     * optimize_sampled() are not affected. */
    void set_loss(int loss, float scale);
    int loss() const { return loss_; }
    float loss_scale() const { return loss_scale_; }
    /* The distance and the voxel weight each of the n points meets under `pose` (source -> map), as a pass from that pose sees
     * them (gsdf_align_residuals): phi and w are resized to n; both are 0 where the voxel is missing.  With pose() after a
     * robust run, |phi| against the loss's scale splits the cloud into what registered and what moved. */
    void residuals(const float* xyz, size_t n, SE3 pose, std::vector<float>& phi, std::vector<float>& w);
};

#endif
