// Do the device's double sin / cos return libm's bits at the arguments of the overlay's exact-ratio table?
// (pose overlay: overlay_segments' six sines come from libm on the host and from the device math library inside
// whenet_overlay_plan_kernel; tests/overlay_lattice_cases.py holds the heads at which one ulp of a sine moves a pixel.)
// Arguments: every float32 multiple of 3 degrees in -180..180 (the lattice's multiples of 15 and the bin centres; -99 and 96 are
// among them) and the next float32 above each (the controls), as overlay_segments forms them: a * pi / 180 and its negation.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/probes/overlay_trig_probe.hip -o tools/probes/overlay_trig_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

__global__ void trig(const double* x, double* s, double* c, int n) {
    const int i = int(blockIdx.x) * int(blockDim.x) + int(threadIdx.x);
    if (i >= n) return;
    s[i] = sin(x[i]);
    c[i] = cos(x[i]);
}

static int64_t bits(double v) {
    int64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

int main() {
    std::vector<double> x;
    std::vector<float> deg;
    const double pi = 3.141592653589793;
    for (int a = -180; a <= 180; a += 3)
        for (int step = 0; step < 2; ++step) {
            const float f = step ? std::nextafterf(float(a), INFINITY) : float(a);
            const double r = double(f) * pi / 180.0;
            x.push_back(r), deg.push_back(f);
            x.push_back(-r), deg.push_back(f);
        }
    const int n = int(x.size());
    double *dx, *ds, *dc;
    if (hipMalloc(&dx, n * 8) != hipSuccess || hipMalloc(&ds, n * 8) != hipSuccess || hipMalloc(&dc, n * 8) != hipSuccess) return 2;
    if (hipMemcpy(dx, x.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess) return 2;
    hipLaunchKernelGGL(trig, dim3((n + 255) / 256), dim3(256), 0, 0, dx, ds, dc, n);
    std::vector<double> s(n), c(n);
    if (hipMemcpy(s.data(), ds, n * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(c.data(), dc, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int differ = 0, differ_lattice = 0;
    for (int i = 0; i < n; ++i) {
        const double hs = std::sin(x[i]), hc = std::cos(x[i]);
        const bool exact_angle = deg[i] == std::rint(deg[i]);
        for (int k = 0; k < 2; ++k) {
            const double h = k ? hc : hs, d = k ? c[i] : s[i];
            if (bits(h) == bits(d)) continue;
            ++differ, differ_lattice += exact_angle;
            printf("%s(%.17g) [%.9g deg%s]: libm %.17g, device %.17g, %lld ulp\n", k ? "cos" : "sin", x[i], double(deg[i]), (i & 1) ? ", negated" : "",
                   h, d, (long long)(bits(d) - bits(h)));
        }
    }
    printf("overlay_trig_probe: %d arguments, %d of %d sin / cos values differ from libm (%d at the multiples of 3 degrees themselves)\n", n, differ,
           2 * n, differ_lattice);
    return 0;
}
