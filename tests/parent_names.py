"""What HotPathDevice and HotPathEnsemble (2 members) of synthetic.hotpath_scenario(48, 60), report=None, held on the commit
before snow and frost came to the device: read from objects built by that commit's code.  tests/test_hotpath_meteo_gpu.py
holds objects without meteo= to these lists."""
# HotPathDevice.state_names(), HotPathEnsemble.state_names() and .analysis_names(), in order
STATE_NAMES = ("Interception TaInterception LeafDrainage CumInterception potential_transpiration RWS Ta W1a W1b W1 "
               "AvailableWaterForInfiltration DSLR ESAct PrefFlow Infiltration W2 Theta1a Theta1b Theta2 Sat1a Sat1b Sat1 Sat2 "
               "SeepTopToSubA SeepTopToSubB SeepSubToGW UZOutflow UZ GwPercUZLZ CumInterSealed LZ LZInflowCUM TaInterceptionCUM "
               "TaCUM ESActCUM GwLossCUM OFQDirect OFQOther OFQForest OFM3Direct OFM3Other OFM3Forest ChanQKin ChanM3Kin Chan2QKin "
               "Chan2M3Kin CrossSection2Area Sideflow1Chan ChanQ sumDisDay").split()
# sorted(HotPathDevice.d)
DEVICE_VECTORS = ("AvailableWaterForInfiltration Chan2M3Kin Chan2M3Start Chan2QKin Chan2QStart ChanLength ChanM3Kin ChanQ ChanQKin "
                  "ChannelAlpha ChannelAlpha2 CropCoef CropGroupNumber CrossSection2Area CumInterSealed CumInterception DSLR "
                  "DirectRunoff DirectRunoffFraction ESAct ESActCUM ESActPixel ESMax ESRef ETRef EWRef EWaterAct FlowVelocity "
                  "GenuInvM1a GenuInvM1b GenuInvM2 GenuM1a GenuM1b GenuM2 GwLossCUM GwLossLZ GwLossStep GwPercStep GwPercUZLZ "
                  "GwPercUZLZPixel Infiltration InfiltrationPixel InterSealed Interception InvChanLength InvChannelAlpha "
                  "InvChannelAlpha2 IsChannel IsChannelKinematic KSat1a KSat1b KSat2 LAI LAITerm LZ LZAvInflow LZInflowCUM LZOutflow "
                  "LZOutflowToChannelPixel LZThreshold LeafDrainage LowerZoneK M3Limit OFAlpha OFM3Direct OFM3Forest OFM3Other "
                  "OFQDirect OFQForest OFQOther OFToChanM3 PixelArea PoreSpaceNotZero1a PoreSpaceNotZero1b PoreSpaceNotZero2 "
                  "PowerInfPot PowerPrefFlow PrefFlow PrefFlowPixel QLimit RWS Rain RainSnowmelt SMaxSealed Sat1 Sat1a Sat1b Sat2 "
                  "SeepSubToGW SeepSubToGWPixel SeepTopToSubA SeepTopToSubB SeepTopToSubPixelA SeepTopToSubPixelB Sideflow1Chan "
                  "SideflowChanM3 SnowMelt SoilDepth1a SoilDepth1b SoilDepth2 SoilDepthTotal SoilFraction StoreMaxPervious "
                  "SurfaceRunSoil SurfaceRunoff TASealed Ta TaCUM TaInterception TaInterceptionAll TaInterceptionCUM TaPixel Theta "
                  "Theta1a Theta1aPixel Theta1b Theta1bPixel Theta2 Theta2Pixel ThetaAll ToChanM3Runoff ToChanM3RunoffDt TotalRunoff "
                  "TravelDistance UZ UZOutflow UZOutflowPixel UpperZoneK W1 W1a W1b W2 WFC1 WFC1a WFC1b WFC2 WRes1 WRes1a WRes1b WRes2 "
                  "WS1 WS1a WS1b WS2 WWP1 WWP1a WWP1b WWP2 WaterDepth WaterFraction b_Xinanjiang isFrozenSoil potential_transpiration "
                  "scratch scratch0 scratch1 sumDisDay").split()
# sorted(HotPathEnsemble.land.dev)
ENSEMBLE_LAND_VECTORS = ("AvailableWaterForInfiltration CropCoef CropGroupNumber CumInterSealed CumInterception DSLR DirectRunoff "
                         "DirectRunoffFraction ESAct ESActCUM ESActPixel ESRef ETRef EWRef EWaterAct GenuInvM1a GenuInvM1b GenuInvM2 GenuM1a "
                         "GenuM1b GenuM2 GwLossCUM GwLossLZ GwLossStep GwPercStep GwPercUZLZ GwPercUZLZPixel Infiltration InfiltrationPixel "
                         "InterSealed Interception IsChannel KSat1a KSat1b KSat2 LAI LAITerm LZ LZAvInflow LZInflowCUM LZOutflow "
                         "LZOutflowToChannelPixel LZThreshold LeafDrainage LowerZoneK OFAlpha OFM3Direct OFM3Forest OFM3Other OFQDirect "
                         "OFQForest OFQOther OFToChanM3 PoreSpaceNotZero1a PoreSpaceNotZero1b PoreSpaceNotZero2 PowerInfPot PowerPrefFlow "
                         "PrefFlow PrefFlowPixel RWS Rain RainSnowmelt SMaxSealed Sat1 Sat1a Sat1b Sat2 SeepSubToGW SeepSubToGWPixel "
                         "SeepTopToSubA SeepTopToSubB SeepTopToSubPixelA SeepTopToSubPixelB SnowMelt SoilDepth1a SoilDepth1b SoilDepth2 "
                         "SoilDepthTotal SoilFraction StoreMaxPervious SurfaceRunSoil SurfaceRunoff TASealed Ta TaCUM TaInterception "
                         "TaInterceptionAll TaInterceptionCUM TaPixel Theta Theta1a Theta1aPixel Theta1b Theta1bPixel Theta2 Theta2Pixel "
                         "ThetaAll ToChanM3Runoff ToChanM3RunoffDt TotalRunoff UZ UZOutflow UZOutflowPixel UpperZoneK W1 W1a W1b W2 WFC1 WFC1a "
                         "WFC1b WFC2 WRes1 WRes1a WRes1b WRes2 WS1 WS1a WS1b WS2 WWP1 WWP1a WWP1b WWP2 WaterDepth WaterFraction b_Xinanjiang "
                         "isFrozenSoil potential_transpiration scratch").split()
