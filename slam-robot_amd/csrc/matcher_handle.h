// matcher_handle.h — the sg_matcher handle: the all-pairs matcher (hamming.hip) and, from the first sg_matcher_db_*
// call on, the keyframe descriptor database (retrieve.hip).  Both work on the handle's one stream and share nothing
// else.
#ifndef SG_MATCHER_HANDLE_H_
#define SG_MATCHER_HANDLE_H_

#include <hip/hip_runtime.h>

#include <memory>

#include "slamgpu.h"

namespace sg {
class HammingMatcher;
class KeyframeDb;
void DeleteKeyframeDb(KeyframeDb* db);   // retrieve.hip
}  // namespace sg

struct sg_matcher {
  std::unique_ptr<sg::HammingMatcher> m;
  sg_device_options dev{};
  hipStream_t stream = nullptr;   // owned by m
  sg::KeyframeDb* db = nullptr;   // created by the first sg_matcher_db_add
  sg_matcher();
  ~sg_matcher();                  // hamming.hip: the database goes before the stream
};

#endif  // SG_MATCHER_HANDLE_H_
