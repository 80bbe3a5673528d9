// map_point_culling.hpp -- the list rule of LocalMapping::MapPointCulling (reference src/vslam/src/LocalMapping.cc:261-297) on flat
// records, host only: no device, no library.  asd_adapters.hpp feeds it MapPoint::Observations() from the observation table
// (asd_map_observations); host/test_map_point_culling.cpp runs it alone.
#ifndef ASD_MAP_POINT_CULLING_HPP
#define ASD_MAP_POINT_CULLING_HPP
#include <cstddef>
#include <cstdint>
#include <vector>

namespace asd {

// one entry of mlpRecentAddedMapPoints
struct RecentMapPoint {
  int32_t row;          // the point's bank row
  int32_t mnFirstKFid;
  int32_t mnFound, mnVisible;
  bool isBad;
};

struct MapPointCullingResult {
  int rc = 0;
  std::vector<size_t> setBad;              // positions in the list given: pMP->SetBadFlag() (:283, :289)
  std::vector<RecentMapPoint> recent;      // mlpRecentAddedMapPoints afterwards, order kept
};

// observations[i] = Observations() of recent[i].  cnThObs = 2: monocular (:268-272).
inline MapPointCullingResult MapPointCullingRule(const std::vector<RecentMapPoint>& recent, const std::vector<int32_t>& observations,
                                                 int32_t nCurrentKFid, int cnThObs = 2) {
  MapPointCullingResult R;
  for (size_t i = 0; i < recent.size(); ++i) {
    const RecentMapPoint& p = recent[i];
    if (p.isBad) continue;                                                   // :277-280
    const float foundRatio = static_cast<float>(p.mnFound) / p.mnVisible;   // MapPoint::GetFoundRatio, in f32 as there
    if (foundRatio < 0.25f) { R.setBad.push_back(i); continue; }             // :281-285
    if (nCurrentKFid - p.mnFirstKFid >= 2 && observations[i] <= cnThObs) { R.setBad.push_back(i); continue; }   // :287-291
    if (nCurrentKFid - p.mnFirstKFid >= 3) continue;                         // :292-293
    R.recent.push_back(p);                                                   // :294-295
  }
  return R;
}

}  // namespace asd
#endif
