// DeviceGroup (group.h): creation, the checks that need no device, the shared-card rule.
#include "group.h"

#include <new>
#include <stdexcept>

#include "codec.h"

namespace ieache {

void DeviceGroup::validate_devices(const int* devices, int n_devices) {
    if (n_devices < 1 || n_devices > kGroupMaxDevices)
        throw std::invalid_argument("n_devices = " + std::to_string(n_devices) + " is outside 1 .. " + std::to_string(kGroupMaxDevices));
    if (!devices) throw std::invalid_argument("null devices list");
    for (int m = 0; m < n_devices; m++)
        if (devices[m] < 0) throw std::invalid_argument("devices[" + std::to_string(m) + "] = " + std::to_string(devices[m]) + " is negative");
}

void DeviceGroup::validate(const Params& p, const int* devices, int n_devices) {
    validate_devices(devices, n_devices);
    if (!p.supported()) throw std::invalid_argument("unsupported parameter set");
}

DeviceGroup::DeviceGroup(const Params& p, const Torus32* bk, const Torus32* ksk, const int* devices, int n_devices) {
    validate(p, devices, n_devices);
    if (!bk || !ksk) throw std::invalid_argument("null key arrays");
    members_.reserve((size_t)n_devices);
    for (int m = 0; m < n_devices; m++) {
        const std::string where = "member " + std::to_string(m) + " (device " + std::to_string(devices[m]) + "): ";
        // a throw leaves through this constructor: members_ and with it the members already made are destroyed
        try {
            std::unique_ptr<ieache_ctx> ctx(new ieache_ctx);
            ctx->eval.reset(new Evaluator(p, devices[m]));
            ctx->eval->load_keys_host(bk, ksk);
            members_.push_back(std::move(ctx));
        } catch (const std::bad_alloc&) {
            throw;
        } catch (const std::invalid_argument& e) {
            throw std::invalid_argument(where + e.what());
        } catch (const std::exception& e) {
            throw std::runtime_error(where + e.what());
        }
    }
    for (size_t m = 0; m < members_.size(); m++)
        if (shares_card(m) && !members_[m]->eval->set_option("br_mix", 0)) throw std::runtime_error(member_label(m) + "br_mix = 0 refused");
}

std::unique_ptr<DeviceGroup> DeviceGroup::from_file(const std::string& cloud_key_path, const int* devices, int n_devices) {
    validate_devices(devices, n_devices);
    CloudKeyData ck;
    load_cloud_key(cloud_key_path, &ck);
    return std::unique_ptr<DeviceGroup>(new DeviceGroup(ck.p, ck.bk.data(), ck.ksk.data(), devices, n_devices));
}

bool DeviceGroup::shares_card(size_t m) const {
    for (size_t j = 0; j < members_.size(); j++)
        if (j != m && device(j) == device(m)) return true;
    return false;
}

std::string DeviceGroup::member_label(size_t m) const {
    return "member " + std::to_string(m) + " (device " + std::to_string(device(m)) + "): ";
}

}  // namespace ieache
