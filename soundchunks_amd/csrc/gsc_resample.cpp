// Crops at a common sample rate and channel count, host side (no HIP): the
// resampler's tables and their process-wide cache, and the host planner of
// gsc_decode_crops and gsc_decode_crops_fmt (per crop: gsc_crop_plan.h).  The
// resampler's definition is in include/soundchunks.h; the kernel that applies
// it is gsc_decode_resample.hip.
#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>

#include "gsc_crop_plan.h"
#include "gsc_decode.h"

namespace gsc {

namespace {

std::string pair_name(int in_rate, int out_rate) {
    return std::to_string(in_rate) + " Hz -> " + std::to_string(out_rate) + " Hz";
}

// the exact Blackman window on |u| <= 1
double window(double u) {
    if (std::fabs(u) > 1.0) return 0.0;
    const double pi = 3.14159265358979323846;
    return 7938.0 / 18608.0 + 9240.0 / 18608.0 * std::cos(pi * u) + 1430.0 / 18608.0 * std::cos(2.0 * pi * u);
}

double sinc(double x) {
    const double pi = 3.14159265358979323846;
    return x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
}

// One phase: taps coefficients for k = -T + 1 .. T, d = k - phase / phases.
void build_row(const ResampleShape& s, int phase, int32_t* row) {
    const int taps = s.taps(), T = s.half_taps;
    const double rho = s.step > s.phases ? double(s.phases) / double(s.step) : 1.0;
    const double W = double(kResampleZeros) / rho;
    std::vector<double> h(static_cast<size_t>(taps));
    double sum = 0.0;
    for (int j = 0; j < taps; ++j) {
        const int k = j - T + 1;
        // k - phase / phases with an exact numerator, so that phase L - p mirrors phase p
        const double d = double(int64_t(k) * s.phases - phase) / double(s.phases);
        h[size_t(j)] = rho * sinc(rho * d) * window(d / W);
        sum += h[size_t(j)];
    }
    const double one = double(int64_t(1) << kResampleShift);
    int64_t total = 0;
    int big = 0;
    for (int j = 0; j < taps; ++j) {
        row[j] = int32_t(std::nearbyint(one * h[size_t(j)] / sum));  // round half even
        total += row[j];
        if (std::fabs(h[size_t(j)]) > std::fabs(h[size_t(big)])) big = j;  // the lowest k on a tie
    }
    row[big] += int32_t((int64_t(1) << kResampleShift) - total);
}

struct Table {
    ResampleShape shape;
    std::vector<int32_t> coeff;
};

}  // namespace

int resample_shape(int in_rate, int out_rate, ResampleShape* shape, std::string* err) {
    auto refuse = [&](const std::string& what) {
        if (err) *err = "gsc resample: " + pair_name(in_rate, out_rate) + ": " + what;
        return -1;
    };
    if (in_rate <= 0 || out_rate <= 0) return refuse("a rate must be positive");
    const int g = std::gcd(in_rate, out_rate);
    ResampleShape s;
    s.phases = out_rate / g;
    s.step = in_rate / g;
    // T = ceil(Z / rho), rho = min(1, Fo / Fi)
    const int64_t T = s.step > s.phases ? (int64_t(kResampleZeros) * s.step + s.phases - 1) / s.phases : kResampleZeros;
    if (2 * T > kResampleMaxTaps)
        return refuse(std::to_string(2 * T) + " taps, more than " + std::to_string(kResampleMaxTaps) +
                      " (the output rate is below 1/16 of the input rate)");
    s.half_taps = int(T);
    const int64_t bytes = int64_t(s.phases) * s.taps() * int64_t(sizeof(int32_t));
    if (bytes > kResampleMaxBytes)
        return refuse("a table of " + std::to_string(s.phases) + " phases x " + std::to_string(s.taps()) +
                      " taps exceeds " + std::to_string(kResampleMaxBytes >> 20) + " MiB");
    if (shape) *shape = s;
    return 0;
}

const int32_t* resample_table(int in_rate, int out_rate, ResampleShape* shape, std::string* err) {
    ResampleShape s;
    if (resample_shape(in_rate, out_rate, &s, err) != 0) return nullptr;
    static std::mutex mu;
    static std::map<std::pair<int, int>, std::unique_ptr<Table>> cache;  // by (phases, step): the reduced pair
    std::lock_guard<std::mutex> lock(mu);
    std::unique_ptr<Table>& t = cache[{s.phases, s.step}];
    if (!t) {
        t.reset(new Table{s, std::vector<int32_t>(size_t(s.phases) * size_t(s.taps()))});
        for (int p = 0; p < s.phases; ++p) build_row(s, p, t->coeff.data() + size_t(p) * size_t(s.taps()));
    }
    if (shape) *shape = s;
    return t->coeff.data();
}

int64_t resample_outputs(int64_t samples, int64_t begin, const ResampleShape& s) {
    if (begin >= samples) return 0;
    return ((samples - begin) * s.phases + s.step - 1) / s.step;
}

int plan_crops(const Index* const* ixs, int nstreams, const Crop* crops, int ncrops, int64_t length, int out_rate,
               int out_channels, CropPlan* plan, std::string* err) {
    *plan = CropPlan();
    auto fail = [&](const std::string& what) {
        if (err) *err = what;
        return -1;
    };
    auto refuse = [&](int i, const std::string& what) {
        return fail("gsc crops: crop " + std::to_string(i) + ": " + what);
    };
    if (!ixs || nstreams <= 0 || ncrops < 0 || (ncrops > 0 && !crops) || length < 0 || out_channels < 0)
        return fail("gsc crops: invalid argument");
    if (out_rate < 0) return fail("gsc resample: output rate " + std::to_string(out_rate) + " Hz: a rate must be positive");
    std::vector<ResampleShape> shapes(static_cast<size_t>(nstreams));
    for (int s = 0; s < nstreams; ++s) {
        if (!ixs[s]) return fail("gsc crops: stream " + std::to_string(s) + " is null");
        const int cs = ixs[s]->channels;
        if (out_channels == 0 && cs != ixs[0]->channels)
            return fail("gsc crops: stream " + std::to_string(s) + " has " + std::to_string(cs) +
                        " channels, stream 0 has " + std::to_string(ixs[0]->channels));
        if (out_channels != 0 && cs != out_channels && cs != 1 && out_channels != 1)
            return fail("gsc crops: stream " + std::to_string(s) + " has " + std::to_string(cs) +
                        " channels, which do not map to " + std::to_string(out_channels) +
                        " (equal counts, a mono stream, or a mono output)");
        // a stream without samples has no rate of its own and is never read
        if (out_rate != 0 && ixs[s]->rate != out_rate && ixs[s]->samples > 0) {
            std::string e;
            if (resample_shape(ixs[s]->rate, out_rate, &shapes[size_t(s)], &e) != 0)
                return fail("gsc crops: stream " + std::to_string(s) + ": " + e);
        }
        const ResampleShape& sh = shapes[size_t(s)];
        if ((int64_t(sh.taps()) + 2) * std::max(cs, 1) > kResampleSrcCap)
            return fail("gsc crops: stream " + std::to_string(s) + ": " + std::to_string(sh.taps()) + " taps x " +
                        std::to_string(cs) + " channels (" + pair_name(ixs[s]->rate, out_rate) +
                        ") exceed the " + std::to_string(kResampleSrcCap) + " source samples of one workgroup");
        // positions are begin * phases + n * step in 64 bits
        if (ixs[s]->samples > (int64_t(1) << 40) || length > (int64_t(1) << 40) / sh.step)
            return fail("gsc crops: stream " + std::to_string(s) + ": too long for one call");
    }
    plan->channels = out_channels ? out_channels : ixs[0]->channels;
    plan->crops.reserve(size_t(ncrops));
    for (int i = 0; i < ncrops; ++i) {
        const Crop& c = crops[i];
        if (crop_stream_status(c.stream, nstreams) != kCropGood)
            return refuse(i, "stream index " + std::to_string(c.stream));
        const Index& ix = *ixs[c.stream];
        const ResampleShape& sh = shapes[size_t(c.stream)];
        CropSpan sp;
        const int status =
            crop_plan_one(c.begin, c.count, length, ix.samples, int32_t(ix.frames.size()), sh.phases, sh.step,
                          sh.half_taps, [&](int32_t f) { return ix.frames[size_t(f)].first_sample; }, &sp);
        if (status == kCropBadBegin)
            return refuse(i, "begin " + std::to_string(c.begin) + " outside [0, " + std::to_string(ix.samples) + "]");
        if (status == kCropBadCount)
            return refuse(i, "count " + std::to_string(c.count) + " outside [0, length " + std::to_string(length) + "]");
        const PlanCrop pc{c.stream,     c.begin,    sp.count,  sp.f0,   sp.f1,
                          sp.src_begin, sp.src_end, sh.phases, sh.step, sh.half_taps};
        plan->crops.push_back(pc);
    }
    return 0;
}

}  // namespace gsc
