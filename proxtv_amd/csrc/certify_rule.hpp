// certify_rule.hpp -- the constants of the certifier's rounding and step rules (reasoning: kernel_certify.hpp), on their own so
// that code which must call the same edges steps (vjpcore.hpp: the derivative of the prox) shares them instead of copying them.
// Plain C++: also compiled by the host harnesses under tests/.
#pragma once

#include "walker.hpp"   // kEps

namespace ptv {
namespace swp {

constexpr double kCertifyTol = 64.0, kCertifyStep = 256.0, kCertifyUlp = 2.220446049250313e-16, kCertifySlack = 4.0 * kEps;

}  // namespace swp
}  // namespace ptv
