// fot_replay.hpp -- the host logic of a replayed closed-loop episode that does not touch the GPU: the replay clock, the
// observer's sampling clock and window, the prepend test and the termination test (fot_loop_set_replay / fot_loop_run).
// Plain C++, no HIP: fot_host_loop.cpp uses it, tests/emu/fot_replay_emu.cpp exposes it to the CPU tests, which hold it
// against closed_loop.py's Observer / ReplayPedestrians / BatchedClosedLoop._loop_frame step by step.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace fot {

// Row of a recording of n_frames frames that replay frame `frame` shows: the last frame is held once the recording
// ends (ReplayPedestrians.step, replay_source.py:86-99).
inline int replay_row(int frame, int n_frames) { return frame < n_frames - 1 ? frame : n_frames - 1; }

// The pedestrians' clock and the observer on it (closed_loop.py _advance_pedestrians + Observer.update,
// src/pedestrian/observer.py:28-102): every frame advances the time by dt; the observer takes a sample whenever
// sgan_dt of pedestrian time has accumulated (with its 1e-9 tolerance) and keeps the last obs_len of them.  A sample is
// remembered as the replay frame it was taken at.
struct ReplayClock {
    int obs_len = 0;
    double dt = 0.0, sgan_dt = 0.0;
    int frame = 0;                           // replay frame counter (not clamped: replay_row clamps per recording)
    double ped_time = 0.0;
    double accumulated = 0.0;                // Observer.accumulated_time
    bool have_update = false;                // Observer._last_update_timestamp is not None
    double last_update = 0.0;
    std::vector<int32_t> sample_frame;       // the window, oldest first (deque(maxlen = obs_len))
    std::vector<double> sample_time;

    void reset(int obs_len_, double dt_, double sgan_dt_)
    {
        obs_len = obs_len_; dt = dt_; sgan_dt = sgan_dt_;
        frame = 0; ped_time = 0.0; accumulated = 0.0; have_update = false; last_update = 0.0;
        sample_frame.clear(); sample_time.clear();
    }
    void advance()
    {
        frame += 1;
        ped_time += dt;
        const double delta = have_update ? std::fmax(ped_time - last_update, 0.0) : dt;
        have_update = true; last_update = ped_time;
        accumulated += delta;
        if (accumulated + 1e-9 >= sgan_dt) {
            if ((int)sample_frame.size() >= obs_len && !sample_frame.empty()) {
                sample_frame.erase(sample_frame.begin()); sample_time.erase(sample_time.begin());
            }
            if (obs_len > 0) { sample_frame.push_back(frame); sample_time.push_back(ped_time); }
            accumulated = std::fmax(accumulated - sgan_dt, 0.0);
        }
    }
    bool ready() const { return (int)sample_frame.size() >= obs_len; }
    int last_frame() const { return ready() && !sample_frame.empty() ? sample_frame.back() : -1; }
    int prev_frame() const { return ready() && sample_frame.size() >= 2 ? sample_frame[sample_frame.size() - 2] : -1; }
    // time since the observer's last sample (integrated_simulator.py:463-470)
    double staleness() const { return sample_time.empty() ? 0.0 : std::fmax(ped_time - sample_time.back(), 0.0); }
};

// Is the first predicted position of a pedestrian away from its current one?  The reference's
// np.allclose(pred[:, 0], current) (integrated_simulator.py:503-511; rtol 1e-5, atol 1e-8) on the first sample of the
// constant-velocity prediction: obs_last + v (dt + staleness), observations rounded to float32 and the velocity formed
// in float32 (trajectory_predictor.py:216).  Every product and sum is a statement of its own: nothing may contract.
inline bool replay_axis_far(double last, double prev, double current, double sgan_dt, double dt, double staleness)
{
    const float l32 = (float)last, p32 = (float)prev;
    const float d32 = l32 - p32;
    const float v32 = d32 / (float)sgan_dt;
    const double zero = 0.0 * dt;
    const double t0 = dt + zero;
    const double t = t0 + staleness;
    const double step = (double)v32 * t;
    const double first = (double)l32 + step;
    const double rel = 1e-5 * std::fabs(current);
    const double tol = 1e-8 + rel;
    return std::fabs(first - current) > tol;
}

// Per episode: do the current positions lead its predicted tracks (any pedestrian away; false without pedestrians)?
// last / prev / current: [P][2] rows of the episode.
inline bool replay_prepend(int P, const double *last, const double *prev, const double *current, double sgan_dt,
                           double dt, double staleness)
{
    bool far = false;
    for (int i = 0; i < 2 * P; ++i) far = replay_axis_far(last[i], prev[i], current[i], sgan_dt, dt, staleness) || far;
    return far;
}

// 0: runs on, 1: collision, 2: goal (integrated_simulator.py:864-883; the collision wins)
inline int replay_termination(int collision, double s_end, double s_now, double goal_distance)
{
    if (collision != 0) return 1;
    return s_end - s_now < goal_distance ? 2 : 0;
}

}  // namespace fot
