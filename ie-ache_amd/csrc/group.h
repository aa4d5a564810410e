// A device group: one cloud key resident on several GPUs of the node, N member contexts behind one handle (include/ieache.h,
// "2b. Device group").  What ieache_group is, and what the daemon keeps its evaluators in.
//
// A member IS an ieache_ctx -- an evaluator, its circuit cache, its flags -- so everything a context can do a member can do,
// and ieache_group_ctx hands it out as one.  The group adds the one parse of the key file, the checks that need no device,
// and the rule for members that share a card; a call is cut over the members by run_sliced (group_run.h), each member
// evaluating its slice of independent rows with its own stream, scratch and key copy.  Nothing crosses devices.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/ieache.h"
#include "circuit_cache.h"
#include "evaluator.h"
#include "params.h"

// The context of the C ABI (capi.cpp implements its entry points).
struct ieache_ctx {
    std::unique_ptr<ieache::Evaluator> eval;
    ieache::CircuitCache circuits{3};  // a caller alternates between a few batch sizes, or toggles exact_fft per call (bench.py's exact leg)
    std::string variant;
    bool fold = false;           // "fold_constants"
    bool level_quantum = true;   // "level_quantum": batch-aware level widths for the slack-balanced circuits
};

// ieache_eval_jobs (include/ieache.h, section 3c) over a device group, exported from the library like the group forms of
// section 2b: every job's batch is cut over the members with ieache_shard_slice (shard_jobs, group_run.h), member m runs
// ieache_eval_jobs on its slices on a host thread of its own -- slices that are empty dropped -- and a member left without
// any does nothing and reports zeros.  The jobs are checked once, on member 0, before any thread starts (the circuits give
// the rows per expression).  stats: NULL or one record per member.  First failing member wins, behind "member M (device D): ";
// the outputs are then unspecified -- no partial output is promised -- and the group stays usable.  A NULL group: IEACHE_EINVAL.
extern "C" int ieache_group_eval_jobs(ieache_group* g, const ieache_job* jobs, size_t n_jobs, ieache_stats* stats /* [n members] or NULL */);

namespace ieache {

constexpr int kGroupMaxDevices = 16;  // IEACHE_GROUP_MAX_DEVICES: the host threads of one call

class DeviceGroup {
public:
    // What can be judged without a device, in this order, each a std::invalid_argument naming the argument: n_devices in
    // 1 .. kGroupMaxDevices, a device list, no negative index, a parameter set Params::supported() accepts.  No HIP call is
    // made, so a machine without a GPU refuses the same arguments the same way.
    static void validate_devices(const int* devices, int n_devices);
    static void validate(const Params& p, const int* devices, int n_devices);

    // validate(), then one member per listed device in list order: Evaluator(p, device), load_keys_host(bk, ksk).  A device may
    // be listed more than once (several contexts on one card).  A member whose device occurs more than once in the list is
    // created with "br_mix" = 0: the rotation of roles assumes the chip to itself (mix_geometry tests ONE evaluator's
    // concurrency), and two contexts on a card would each open three streams for it.  Output bits do not depend on the
    // option.  If a member cannot be made, the ones already made are destroyed and the exception names member and device.
    DeviceGroup(const Params& p, const Torus32* bk, const Torus32* ksk, const int* devices, int n_devices);
    // the key file parsed ONCE (load_cloud_key), whatever the number of members; the device list is judged before it is read
    static std::unique_ptr<DeviceGroup> from_file(const std::string& cloud_key_path, const int* devices, int n_devices);

    size_t size() const { return members_.size(); }
    ieache_ctx* member(size_t m) const { return members_[m].get(); }
    int device(size_t m) const { return members_[m]->eval->device(); }
    bool shares_card(size_t m) const;  // its device index occurs more than once in the list
    // "member M (device D): " -- how a failure inside a group call names where it happened
    std::string member_label(size_t m) const;

private:
    std::vector<std::unique_ptr<ieache_ctx>> members_;  // in list order; each evaluator idles its own streams before it goes
};

}  // namespace ieache
