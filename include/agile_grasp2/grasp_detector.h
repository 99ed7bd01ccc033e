// grasp_detector.h -- host mirror of GraspDetector (include/agile_grasp2/grasp_detector.h:68-168,
// src/agile_grasp2/grasp_detector.cpp).  The ros::NodeHandle of the reference constructor is
// replaced by a plain Params struct carrying exactly the ROS parameter names and defaults of
// grasp_detector.cpp:19-80 (plus readers for "key=value" text and roslaunch <param> XML).
#ifndef AGILE_GRASP2_GRASP_DETECTOR_H
#define AGILE_GRASP2_GRASP_DETECTOR_H

#include <memory>
#include <string>
#include <vector>

#include "agile_grasp2/caffe_classifier.h"
#include "agile_grasp2/cloud_camera.h"
#include "agile_grasp2/grasp_hypothesis.h"
#include "agile_grasp2/hand_search.h"
#include "agile_grasp2/handle_search.h"
#include "agile_grasp2/learning.h"
#include "agile_grasp2/messages.h"

class GraspDetector {
 public:
  static const int NONE = 0, PREDICTION = 1, GEOMETRIC = 2;   // antipodal_mode, grasp_detector.cpp:5-7
  static const int NO_PLOTTING = 0, PCL = 1, RVIZ = 2;        // plot_mode (accepted, ignored)

  struct Params {  // names and defaults: grasp_detector.cpp:19-80
    std::vector<double> workspace;     // no default in the reference
    std::vector<double> camera_pose;   // 16 values row-major, or empty => Baxter defaults (:108-126)
    int num_samples = 1000;
    std::vector<int> sample_indices;
    int num_threads = 1;
    double nn_radius_taubin = 0.01;
    double nn_radius_hands = 0.1;
    int num_orientations = 8;
    bool voxelize = true;
    bool filter_half_grasps = true;
    double finger_width = 0.01;
    double hand_outer_diameter = 0.09;
    double hand_depth = 0.06;
    double hand_height = 0.02;
    double init_bite = 0.015;
    int antipodal_mode = PREDICTION;
    std::string model_file, trained_file, label_file;
    double min_score_diff = 500.0;
    int batch_size = 10;               // accepted; the GPU path scores all images in one batch
    int min_inliers = 0;               // > 0: HandleSearch::findClusters before the top-k (grasp_detector.cpp:59-65,228-236)
    double min_length = 0.005;
    bool reuse_inliers = true;
    int num_selected = 50;
    std::vector<double> gripper_width_range{0.03, 0.07};
    int plot_mode = NO_PLOTTING;
    bool only_plot_output = true;
    // not in the reference
    int device = 0;
    uint64_t seed = 0;
    // More than one entry: detectGraspPoses (antipodal_mode PREDICTION, index samples) spreads the sample list
    // over these GPUs -- one context and one host thread per entry, the cloud replicated, every device taking a
    // contiguous range of the samples (they are independent, hand_search.cpp:194-228) --, gathers the ranks'
    // scored candidates on the first device (peer copies over xGMI) and clusters / selects there
    // (grasp_detector.cpp:228-252).  The same device may appear more than once.  Empty: {device}.
    std::vector<int> devices;
    // How `devices` share the work.  TILING_REPLICATE (default): every device holds the whole cloud and takes a
    // contiguous range of the sample list.  TILING_SPATIAL (BASELINE configuration 4, "the cloud shards by
    // spatial tile"): the sample list is put in ascending order along the cloud's longest axis ONCE -- for any
    // number of devices, one included, so the result does not depend on it --, cut into contiguous ranges of
    // equal summed neighbour counts, and every device holds only the points of its samples' interval +- the halo
    // (nn_radius_hands + normals radius), binned against the whole cloud's minimum (ag2_set_grid_origin): grid
    // and normals shard too.  The hypotheses are those of one device running the ordered list
    // (hand_search.cpp:194-228: no state crosses samples).
    enum { TILING_REPLICATE = 0, TILING_SPATIAL = 1 };
    int tiling = TILING_REPLICATE;
    // "name=value" lines ('#' comments); vectors as "[a, b, c]".  Unknown names are an error.
    static bool fromKeyValueText(const std::string& text, Params* out, std::string* err);
    // <param name=".." value=".."/> and <rosparam param=".."> [..] </rosparam> of a roslaunch file
    static bool fromLaunchXml(const std::string& xml, Params* out, std::string* err);
  };

  explicit GraspDetector(const Params& params);
  ~GraspDetector();

  // grasp_detector.cpp:84-282 (PREDICTION: hypotheses -> prune -> images -> LeNet -> threshold ->
  // top-k by score; GEOMETRIC: keep full-antipodal; NONE: pruned hypotheses).  Empty vector for
  // an empty cloud (:86-91) or on error (message on stderr).
  std::vector<GraspHypothesis> detectGraspPoses(const CloudCamera& cloud_cam, bool clusters_grasps = true);
  // grasp_detector.cpp:285-350
  void preprocessPointCloud(CloudCamera& cloud_cam);
  // One frame of a sensor stream, as a live topic needs it (the reference's topic path,
  // grasp_detection_node.cpp:123-143, calls detectGraspPoses on the cloud as it arrives; its file path :97-121
  // preprocesses first): preprocessPointCloud -- workspace filter, voxel grid, uniform sub-sampling of
  // num_samples points -- followed by detectGraspPoses, in ONE GPU call (ag2_detect_frame_raw: filter, voxel
  // grid, sub-sampling and the whole per-frame pipeline in one captured sequence, one host synchronisation).
  // The same hands as the two calls on a CloudCamera of this cloud.  Needs what those calls need for the GPU
  // front end: one camera, voxelize, no incoming samples or indices, antipodal_mode PREDICTION; any other
  // setting takes the two calls.
  std::vector<GraspHypothesis> detectGraspPosesInFrame(const PointCloudRGB::Ptr& raw_cloud);
  // One frame of the robot launch file's stream (launch/robot_detect_grasps.launch:4-6): a two-camera CloudSized
  // cloud (grasp_detection_node.cpp:239-259) -- or, second overload, one that brings its normals (:220-226,243-248;
  // the hand search then skips calculateNormalsOMP, hand_search.cpp:20,25-29) -- taken as it arrives, without
  // preprocessPointCloud, with the samples of the detector's index list (setIndicesFromMsg; the topic path :123-143
  // and the find_grasps service :177-193).  The same hands as CloudCamera(cloud, size_left_cloud) + setSampleIndices
  // + detectGraspPoses, in ONE GPU call (ag2_detect_frame_desc: camera mask and normals packed on the device, the
  // per-frame pipeline in one captured sequence).  With indices set the prune is skipped (grasp_detector.cpp:150-160).
  // No indices: nothing, as the topic path.  Outside antipodal_mode PREDICTION, with several devices, incoming
  // samples, or size_left_cloud == size (the one-camera constructor's all-zero camera matrix): the three calls.
  std::vector<GraspHypothesis> detectGraspPosesInFrame(const PointCloudRGB::Ptr& cloud, int size_left_cloud);
  std::vector<GraspHypothesis> detectGraspPosesInFrame(const PointCloudNormal::Ptr& cloud, int size_left_cloud);

  static bool isScoreGreater(const GraspHypothesis& a, const GraspHypothesis& b) {
    return a.getScore() > b.getScore();
  }
  bool getUseIncomingSamples() const { return use_incoming_samples_; }
  void setUseIncomingSamples(bool v) { use_incoming_samples_ = v; }
  const std::vector<double>& getWorkspace() const { return p_.workspace; }
  int getNumSamples() const { return num_samples_; }
  void setNumSamples(int n) { num_samples_ = n; }
  void setIndicesFromMsg(const agile_grasp2::CloudIndexed& msg);               // grasp_detector.h:111, .cpp:353-361
  void setSamplesMsg(const agile_grasp2::SamplesMsg& msg) { samples_msg_ = msg; }
  // grasp_detector.h:123.  The clustering step of detectGraspPoses reads getMinInliers() from this
  // object (grasp_detector.cpp:228-236), so a caller may change it between calls as in the reference.
  HandleSearch& getHandleSearch() { return handle_search_; }

  // grasp_detection_node.cpp:296-313 (createGraspListMsg)
  static agile_grasp2::GraspListMsg createGraspListMsg(const std::vector<GraspHypothesis>& hands);
  // find_grasps service body (grasp_detection_node.cpp:146-201) with the response FILLED -- the
  // reference returns true without filling it (":196 TODO"); documented divergence.
  bool findGrasps(const CloudCamera& cloud_in, const agile_grasp2::FindGraspsRequest& req,
                  agile_grasp2::FindGraspsResponse* resp);

  // not in the reference: the camera poses detectGraspPoses hands to the hand search
  // (grasp_detector.cpp:108-137: the launch file's camera_pose, else the 2-camera Baxter defaults)
  void cameraPoses(ag2::Matrix4d* left, ag2::Matrix4d* right) const;
  // Params::tiling == TILING_SPATIAL: the sample list in ascending order along `*axis` (the cloud's longest extent),
  // stable -- the order every number of devices shards (agile_grasp2_amd/sharding.py: order_samples_by_x)
  static std::vector<int32_t> orderSamplesAlongLongestAxis(const CloudCamera& cloud_cam, const std::vector<int32_t>& idx,
                                                           int* axis);
  // points every device of the last N-device run held (TILING_SPATIAL: its tile; else the whole cloud)
  const std::vector<size_t>& lastTilePoints() const { return tile_points_; }
  const ag2_times& lastStageTimes() const { return times_; }
  const ag2_counters& lastCounters() const { return counters_; }
  const std::string& lastError() const { return err_; }

 protected:
  // detectGraspPoses with the two things ImportanceSampling needs: samples given as xyz regardless
  // of use_incoming_samples_, and "the context already holds this cloud and its normals" (the
  // reference rebuilds the kd-tree and recomputes every normal on each re-entry, hand_search.cpp:11-29)
  // `importance` (index samples, one device, PREDICTION): the whole importance-sampling loop in one
  // ag2_detect_importance call in place of the one detect; its rounds and report are left in *importance.
  struct DeviceImportance {
    ag2_importance_params prm{};
    std::vector<double> rounds;  // rounds x (3 x num_samples), as ag2_get_importance_rounds
    ag2_importance_info info{};
    bool ran = false;
  };
  std::vector<GraspHypothesis> detectImpl(const CloudCamera& cloud_cam, bool clusters_grasps,
                                          const ag2::Matrix3Xd* samples_xyz, bool cloud_is_resident,
                                          DeviceImportance* importance = nullptr);
  const Params& params() const { return p_; }
  std::shared_ptr<ag2::Context> context() const { return ctx_; }

 private:
  std::vector<GraspHypothesis> pruneGraspsOnHandParameters(const std::vector<GraspHypothesis>& hands,
                                                           float min_x, float max_x, float min_y,
                                                           float max_y, float min_z);
  std::shared_ptr<ag2::Context> contextFor(int n_cams);
  ag2_params abiParams(int n_cams) const;
  // the multi-GPU form of step 1 - 5 (Params::devices); false: error (err_ says what)
  bool detectOnDevices(const CloudCamera& cloud_cam, const std::vector<int32_t>& idx, bool do_prune,
                       int min_inliers, std::vector<ag2_hypothesis>* recs, size_t* n);

  bool preprocessOnDevice(CloudCamera& cloud_cam);
  // the sized frame of either record type; false: the caller takes the three calls
  bool sizedFrameOnDevice(const ag2_cloud_desc& cloud, std::vector<GraspHypothesis>* out);

  Params p_;
  int num_samples_;
  std::vector<int> indices_;
  bool use_incoming_samples_ = false;
  double voxel_size_ = 0.003;  // grasp_detector.cpp:15
  agile_grasp2::SamplesMsg samples_msg_;
  std::unique_ptr<Classifier> classifier_;
  std::unique_ptr<Learning> learning_;
  HandleSearch handle_search_;
  std::shared_ptr<ag2::Context> ctx_;
  int ctx_cams_ = 0;
  std::vector<std::shared_ptr<ag2::Context>> peers_;  // contexts of Params::devices[1 ...]
  std::vector<size_t> tile_points_;
  int peers_cams_ = 0;
  // cloud left in the context by preprocessPointCloud: detectGraspPoses does not upload it again
  const void* resident_cloud_ = nullptr;
  size_t resident_n_ = 0;
  const ag2_ctx* resident_ctx_ = nullptr;
  bool resident_normals_ = false;
  bool resident_uploaded_here_ = false;  // by detectImpl (re-entries only), not by preprocessPointCloud
  ag2_times times_{};
  ag2_counters counters_{};
  std::string err_;
};

#endif  // AGILE_GRASP2_GRASP_DETECTOR_H
